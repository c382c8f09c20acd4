#!/usr/bin/env python3
"""Ray queries (rvpt_hip_read with FORMAT_RAY_HITS; Context.trace_rays_into) measured -> profiles/ray_queries.txt.

usage: tools/bench_rays.py rates [default cornell terrain]     on the GPU box: rays/s for the 1920 x 1080 pinhole camera rays of each scene — in pixel order and in a
                                                               random permutation, from host records and from device records, closest hit and any hit with tmax =
                                                               half the scene extent — beside two yardsticks taken in the same run: the context's own frame kernel on
                                                               the same camera with max_bounces = 1 (one segment per sample: primaries only), in segments/s, and
                                                               oracle.closest_hit on this CPU
       tools/bench_rays.py queries [scene]                     a few device-record queries and nothing else: the run to put under rocprofv3
       tools/bench_rays.py resources <parent tree>             where hipcc and a checkout of the parent commit are: VGPR, SGPR, scratch and static LDS of every frame
                                                               kernel there and here (tools/kernel_resources.py), and of the query kernels
       tools/bench_rays.py nearest <label> [scenes]            k-nearest queries (FORMAT_RAY_HITS_NEAREST(k)) on the same 2 M camera rays from device records: k = 1, 2, 4
                                                               and 8 beside format 2 in the same run — Grays/s, hits returned per second, and the ratio to k sequential
                                                               format-2 calls.  <label> names the block the run writes ("this tree", "parent, before", ...); with
                                                               RVPT_HIP_LIB naming a library that has no such format (the parent commit's) the block holds format 2
                                                               alone, three passes, which is the yardstick for format 2's own rate
       tools/bench_rays.py --crossings <label> [scenes]        crossing queries (FORMAT_RAY_CROSSINGS) on the same 2 M camera rays from device records: format 2 in three passes
                                                               and any-hit hits=8 as yardsticks of the same run, format 8 with tmax = inf and with tmax = one scene extent,
                                                               the mean front + back per ray, and how many rays a brute-force context of the same triangles counts
                                                               differently.  With RVPT_HIP_LIB naming a library that has no such format (the parent commit's) the block
                                                               holds the yardsticks alone.  Writes the block of its label into profiles/ray_crossings.txt
Each mode rewrites its own section of profiles/ray_queries.txt and leaves the others; `nearest` rewrites the block of its label inside its section."""
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "profiles" / "ray_queries.txt"
MARK = "==== kernel resources"
W, H = 1920, 1080


MARK_NEAREST = "==== k nearest hits"
BLOCK = "---- block: "


def write_section(text, resources):
    old = OUT.read_text() if OUT.exists() else ""
    old, sep, nearest = old.partition(MARK_NEAREST)  # (the last section: kept as it is)
    nearest = ("\n" + sep + nearest) if sep else ""
    head, _, tail = old.partition(MARK)
    if resources:
        OUT.write_text(head.rstrip("\n") + ("\n\n" if head.strip() else "") + MARK + text.rstrip("\n") + "\n" + nearest)
    else:
        OUT.write_text(text.rstrip("\n") + "\n" + ("\n" + MARK + tail.rstrip("\n") + "\n" if tail else "") + nearest)


def write_nearest_block(label, text):
    """the block `label` of the k-nearest section replaced (or added behind the others); everything in front of the section stays"""
    old = OUT.read_text() if OUT.exists() else ""
    front, _, section = old.partition(MARK_NEAREST)
    blocks = {}
    for part in section.split(BLOCK)[1:]:
        name, _, body = part.partition(" ----\n")
        blocks[name] = body.rstrip("\n")
    blocks[label] = text.rstrip("\n")
    out = front.rstrip("\n") + "\n\n" + MARK_NEAREST + " (tools/bench_rays.py nearest <label>: one block per process, in the order they ran) ====\n"
    for name, body in blocks.items():
        out += "\n" + BLOCK + name + " ----\n" + body + "\n"
    OUT.write_text(out)


def scenes(names):
    from rvpt_amd import Camera, native, scene
    for name in names:
        c = Camera(W / H)
        if name == "default":
            tris, mats = scene.default_scene()
            c.translation = np.array([0.0, 0.8, -1.5])
        elif name == "cornell":
            tris, mats = scene.cornell_scene()
            c.translation = np.array([0.0, 2.0, -1.9])
        else:
            tris, mats = scene.heightfield_scene()
            c.translation = np.array([0.0, 2.5, -5.0])
            c.rotation = np.array([0.0, 25.0, 0.0])
        nodes, idx = native.build_bvh(tris)
        yield name, tris[idx], mats, nodes, c.get_data()


def camera_records(cam, tmax=np.inf, flags=0):
    """the pixel-centre rays of the pinhole camera `cam` (camera.glsl:29-51, float32, made on the host), in pixel order"""
    from rvpt_amd import native
    cam = np.asarray(cam, dtype=np.float32)
    m = cam[:16].reshape(4, 4).T
    x, y = np.meshgrid((np.arange(W, dtype=np.float32) + 0.5) / W, 1.0 - (np.arange(H, dtype=np.float32) + 0.5) / H)
    u, v, w = cam[16] * (2 * x - 1), 2 * y - 1, np.float32(1.0 / np.tan(0.5 * cam[17]))
    d = u[..., None] * m[:3, 0] + v[..., None] * m[:3, 1] + w * m[:3, 2]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rec = np.zeros(W * H, dtype=native.RAY_HIT_DTYPE)
    rec["org"], rec["dir"], rec["tmax"], rec["flags"] = m[:3, 3], d.reshape(-1, 3).astype(np.float32), tmax, flags
    return rec


def rate(fn, n_rays, reps=7, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    r = [n_rays / t / 1e6 for t in ts]
    return f"median {statistics.median(r):9.1f}   min {min(r):9.1f}   max {max(r):9.1f}   Mrays/s (wall clock of the call, n {reps})"


def rates(names):
    import torch
    from oracle import oracle
    from rvpt_amd import RenderSettings, native
    lines = ["ray queries: tools/bench_rays.py rates " + " ".join(names), f"1920 x 1080 pinhole camera rays = {W * H} records per call; one MI355X; rates are wall clock around the call (it returns after its stream has finished)", ""]
    for name, tris, mats, nodes, cam in scenes(names):
        ext = float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
        lines.append(f"== {name}: {tris.shape[0]} triangles, {nodes.shape[0]} nodes, extent {ext:.2f} ==")
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH | native.COUNT_SEGMENTS)
        ctx.upload_scene(nodes, tris, mats)
        order = np.random.RandomState(1).permutation(W * H)
        for what, kw in (("closest hit", {}), (f"any hit, tmax = extent / 2 = {ext / 2:.2f}", {"tmax": np.float32(ext / 2), "flags": native.RAY_ANY_HIT})):
            pixel = camera_records(cam, **kw)
            for oname, rec in (("pixel order", pixel), ("random permutation", np.ascontiguousarray(pixel[order]))):
                dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
                lines.append(f"{what:36s} {oname:20s} host records    {rate(lambda: ctx.trace_rays_into(rec), W * H)}")
                lines.append(f"{what:36s} {oname:20s} device records  {rate(lambda: ctx.trace_rays_into(dev), W * H)}")
                got = dev.cpu().numpy().view(native.RAY_HIT_DTYPE).reshape(-1)
                assert got.tobytes() == rec.tobytes(), "host and device records differ"
                lines.append(f"{'':36s} {'':20s} hits: {int((rec['prim'] != native.NO_PRIM).sum())} of {W * H}")
        # yardstick 1: the context's own frame kernel, primaries only
        frames = 16
        def primaries():
            for f in range(frames):
                ctx.set_frame(RenderSettings(max_bounces=1, aa=1, current_frame=f).pack(), cam)
                ctx.dispatch()
            ctx.wait()
        primaries()
        s0 = ctx.stats()[0]
        t0 = time.perf_counter()
        primaries()
        dt = time.perf_counter() - t0
        seg = ctx.stats()[0] - s0
        lines.append(f"yardstick: frame kernel (variant {ctx.launch_info()[2]}), max_bounces = 1, aa = 1, {frames} one-frame launches: {seg} segments in {dt * 1e3:.2f} ms = {seg / dt / 1e6:.1f} Msegments/s")
        ctx.close()
        # yardstick 2: the oracle on this CPU (one call per ray; every call prepares the scene again, so few rays on the large scene)
        n_cpu = 200 if tris.shape[0] < 100000 else 8
        pick = camera_records(cam)[np.random.RandomState(2).randint(0, W * H, n_cpu)]
        t0 = time.perf_counter()
        for r in pick:
            oracle.closest_hit(nodes, tris, oracle.TRAVERSAL_BVH, r["org"], r["dir"])
        dt = time.perf_counter() - t0
        lines.append(f"yardstick: oracle.closest_hit on this CPU, {n_cpu} rays, one call each (a call prepares the scene's triangles first): {n_cpu / dt:.1f} rays/s")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    write_section(text, resources=False)


def nearest(label, names):
    import torch
    from rvpt_amd import native
    lib = os.environ.get("RVPT_HIP_LIB", "librvpt_hip.so (this tree's)")
    n = W * H
    lines = [f"library: {Path(lib).name}; {n} pixel-centre camera rays in pixel order, closest hit, tmax = inf, device records; wall clock around the call, 7 calls after 2",
             "Grays/s counts rays; a k-nearest call takes n * k records.  `k x format 2` is k format-2 calls on the same records one after the other, timed together:",
             "what a caller who re-traces pays at the least (the new origins are not even made).", ""]

    def timed(fn, reps=7, warm=2):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    for name, tris, mats, nodes, cam in scenes(names):
        lines.append(f"== {name}: {tris.shape[0]} triangles ==")
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
        ctx.upload_scene(nodes, tris, mats)
        rec = camera_records(cam)
        dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
        for p in range(3):  # format 2's own rate, three passes: the figure that is compared with the parent commit's library
            med, lo, hi = timed(lambda: ctx.trace_rays_into(dev))
            lines.append(f"format 2, pass {p + 1}:            median {n / med / 1e9:7.3f}   min {n / hi / 1e9:7.3f}   max {n / lo / 1e9:7.3f}   Grays/s")
        t2 = med
        try:
            ctx.trace_rays_into(dev[:8].clone(), hits=2)
            has_form = True
        except native.NativeError as e:
            has_form = False
            lines.append(f"no k-nearest form in this library ({str(e)[:60]}): format 2 alone")
        for k in (1, 2, 4, 8) if has_form else ():
            groups = np.zeros((n, k), dtype=native.RAY_HIT_DTYPE)
            groups[:, 0] = rec
            devk = torch.from_numpy(groups.view(np.float32).reshape(-1, 12)).to("cuda:0")
            med, lo, hi = timed(lambda: ctx.trace_rays_into(devk, hits=k))
            seq, _, _ = timed(lambda: [ctx.trace_rays_into(dev) for _ in range(k)], reps=5, warm=1)
            got = devk.cpu().numpy().view(native.RAY_HIT_DTYPE).reshape(n, k)
            held = int((got["prim"] != native.NO_PRIM).sum())
            lines.append(f"k = {k}: median {n / med / 1e9:7.3f}   min {n / hi / 1e9:7.3f}   max {n / lo / 1e9:7.3f}   Grays/s   {held} hits returned = {held / med / 1e9:7.3f} Ghits/s   "
                         f"{k} x format 2: {seq * 1e3:8.2f} ms against {med * 1e3:8.2f} ms = {seq / med:5.2f} x   (format 2 alone: {t2 * 1e3:.2f} ms)")
            del devk, groups, got
        ctx.close()
        lines.append("")
    text = "\n".join(lines)
    print(text)
    write_nearest_block(label, text)


OUT_CROSSINGS = ROOT / "profiles" / "ray_crossings.txt"
MARK_CROSSINGS = "==== measured"


def write_crossings_block(label, text):
    """the block `label` of profiles/ray_crossings.txt's measured section replaced (or added behind the others); everything in front of the section stays"""
    old = OUT_CROSSINGS.read_text() if OUT_CROSSINGS.exists() else ""
    front, _, section = old.partition(MARK_CROSSINGS)
    blocks = {}
    for part in section.split(BLOCK)[1:]:
        name, _, body = part.partition(" ----\n")
        blocks[name] = body.rstrip("\n")
    blocks[label] = text.rstrip("\n")
    out = front.rstrip("\n") + "\n\n" + MARK_CROSSINGS + " (tools/bench_rays.py --crossings <label>: one block per process, in the order they ran) ====\n"
    for name, body in blocks.items():
        out += "\n" + BLOCK + name + " ----\n" + body + "\n"
    OUT_CROSSINGS.write_text(out)


def crossings(label, names):
    import torch
    from rvpt_amd import native
    lib = os.environ.get("RVPT_HIP_LIB", "librvpt_hip.so (this tree's)")
    n = W * H
    lines = [f"library: {Path(lib).name}; {n} pixel-centre camera rays in pixel order, device records; wall clock around the call; every figure is the median (min .. max)",
             "of 7 calls after 2, in Grays/s", ""]

    def timed(fn, reps=7, warm=2):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    def figure(t):
        med, lo, hi = t
        return f"{n / med / 1e9:7.3f} ({n / hi / 1e9:7.3f} .. {n / lo / 1e9:7.3f})"

    for name, tris, mats, nodes, cam in scenes(names):
        ext = float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
        lines.append(f"== {name}: {tris.shape[0]} triangles, extent {ext:.2f} ==")
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
        ctx.upload_scene(nodes, tris, mats)
        rec = camera_records(cam)
        dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
        for p in range(3):  # format 2's own rate, three passes: the figure that is compared with the parent commit's library
            t2 = timed(lambda: ctx.trace_rays_into(dev))
            lines.append(f"format 2, pass {p + 1}:                      {figure(t2)}")
        groups = np.zeros((n, 8), dtype=native.RAY_HIT_DTYPE)
        groups[:, 0] = camera_records(cam, flags=native.RAY_ANY_HIT)
        dev8 = torch.from_numpy(groups.view(np.float32).reshape(-1, 12)).to("cuda:0")
        t8 = timed(lambda: ctx.trace_rays_into(dev8, hits=8))
        lines.append(f"any hit, hits=8:                       {figure(t8)}")
        del dev8, groups
        if not hasattr(native, "FORMAT_RAY_CROSSINGS"):
            has_form = False
        else:
            try:
                ctx.count_crossings_into(dev[:8].clone())
                has_form = True
            except native.NativeError as e:
                has_form = False
                lines.append(f"no crossing form in this library ({str(e)[:60]}): the yardsticks alone")
        if has_form:
            tc = timed(lambda: ctx.count_crossings_into(dev))
            got = dev.cpu().numpy().view(native.RAY_CROSSINGS_DTYPE).reshape(-1)
            total = got["front"].astype(np.int64) + got["back"]
            lines.append(f"format 8, tmax = inf:                  {figure(tc)}   = {t2[0] / tc[0]:5.2f} x format 2's rate, {t8[0] / tc[0]:5.2f} x any-hit hits=8's")
            lines.append(f"    front + back per ray: mean {total.mean():.3f}, max {int(total.max())}; rays with a crossing: {int((total > 0).sum())}")
            cut = camera_records(cam, tmax=np.float32(ext))
            devc = torch.from_numpy(cut.view(np.float32).reshape(-1, 12)).to("cuda:0")
            tf = timed(lambda: ctx.count_crossings_into(devc))
            gotc = devc.cpu().numpy().view(native.RAY_CROSSINGS_DTYPE).reshape(-1)
            lines.append(f"format 8, tmax = extent = {ext:7.2f}:      {figure(tf)}   = {t2[0] / tf[0]:5.2f} x format 2's rate; front + back per ray: mean "
                         f"{(gotc['front'].astype(np.int64) + gotc['back']).mean():.3f}")
            # the same triangles on a brute-force context: how many rays get other counts (recorded, not asserted; as many rays as 2e10 triangle tests allow)
            stride = max(1, int(np.ceil(n * float(tris.shape[0]) / 2e10)))
            some = np.ascontiguousarray(rec[::stride])
            brute = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
            brute.upload_scene(None, tris, mats)
            b = brute.count_crossings_into(some.view(native.RAY_CROSSINGS_DTYPE).copy())
            brute.close()
            g = got[::stride]
            differ = int(((b["front"] != g["front"]) | (b["back"] != g["back"])).sum())
            lines.append(f"    BVH context against a brute-force context of the same triangles, every {stride}th ray ({some.shape[0]} rays): {differ} rays with other counts")
            del devc
        ctx.close()
        lines.append("")
    text = "\n".join(lines)
    print(text)
    write_crossings_block(label, text)


def queries(names):
    import torch
    from rvpt_amd import native
    for name, tris, mats, nodes, cam in scenes(names):
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
        ctx.upload_scene(nodes, tris, mats)
        dev = torch.from_numpy(camera_records(cam).view(np.float32).reshape(-1, 12)).to("cuda:0")
        for _ in range(8):
            ctx.trace_rays_into(dev)
        ctx.close()
        print(f"{name}: 8 queries of {W * H} device records done")


def resources(parent):
    import importlib.util

    def tables(root, files=None):
        for k in [k for k in sys.modules if k == "rvpt_amd" or k.startswith("rvpt_amd.")]:
            del sys.modules[k]
        sys.path.insert(0, str(root))
        try:
            spec = importlib.util.spec_from_file_location("kernel_resources", Path(root) / "tools" / "kernel_resources.py")
            m = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(m)
            return m.kernel_resources(files) if files else m.kernel_resources()
        finally:
            sys.path.remove(str(root))

    def table(title, res):
        out = [title, f"  {'kernel':88s} {'vgpr':>5s} {'sgpr':>5s} {'scratch':>8s} {'static_lds':>10s}"]
        for k in sorted(res):
            v = res[k]
            out.append(f"  {k[:88]:88s} {v['vgpr']:5d} {v['sgpr']:5d} {v['scratch_bytes']:8d} {v['static_lds_bytes']:10d}")
        return out

    before, after = tables(parent), tables(ROOT)
    lines = [" (tools/bench_rays.py resources <parent tree>; tools/kernel_resources.py: the compiler's own metadata) ====", ""]
    lines += table("frame kernels, parent commit (rvpt_kernels.hip, rvpt_packets.hip, rvpt_bvh4.hip)", before) + [""]
    lines += table("frame kernels, this commit", after) + [""]
    lines += [f"identical: {before == after} ({len(after)} kernels)", ""]
    lines += table("query kernels (rvpt_query.hip)", tables(ROOT, ["rvpt_query.hip"]))
    text = "\n".join(lines) + "\n"
    print(MARK + text)
    write_section(text, resources=True)
    return before == after


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rates"
    if mode == "resources":
        sys.exit(0 if resources(sys.argv[2]) else 1)
    if mode in ("--crossings", "crossings"):
        crossings(sys.argv[2], sys.argv[3:] or ["default", "cornell", "terrain"])
        sys.exit(0)
    if mode == "nearest":
        nearest(sys.argv[2], sys.argv[3:] or ["default", "cornell", "terrain"])
        sys.exit(0)
    names = sys.argv[2:] or ["default", "cornell", "terrain"]
    rates(names) if mode == "rates" else queries(names)
