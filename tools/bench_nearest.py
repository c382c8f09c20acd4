#!/usr/bin/env python3
"""Point queries (rvpt_hip_read with FORMAT_NEAREST_POINTS; Context.closest_points_into) measured -> profiles/nearest_points.txt.

usage: tools/bench_nearest.py rates [default cornell terrain]   on the GPU box: points/s for 2^20 points of each scene — on a jittered grid through the scene's box
                                                                (near the surface) and on a sphere 10 extents away (the far case, where pruning is worst), from
                                                                host records and from device records — beside the yardsticks of the same run: nearest_brute on a
                                                                brute-force context (the two scenes where that is practical), the ray query's closest-hit rate on
                                                                the same context (rays from the same points towards the scene's centre), and scene.closest_points
                                                                on this CPU for a small n.  The terrain is asked after build_scene("sah"), the others after the host
                                                                build.
       tools/bench_nearest.py queries [scene] [near|far]        a few device-record queries and nothing else: the run to put under rocprofv3
       tools/bench_nearest.py resources <parent tree>           where hipcc and a checkout of the parent commit are: VGPR, SGPR, scratch and static LDS of every
                                                                kernel of every .hip file there and here (tools/kernel_resources.py), and of the new kernels
       tools/bench_nearest.py --k <label> [scenes]              k-nearest point queries (FORMAT_NEAREST_POINTS_K(k)): Gpoints/s of 2^20 near points from device
                                                                records at k = 1, 2, 4, 8 on the three scenes, beside format 4's own rate in three passes.  <label>
                                                                names the block ("this tree", "parent"); with RVPT_HIP_LIB naming a library that has no such format
                                                                (the parent commit's) the block holds format 4 alone.  Blocks are appended to
                                                                profiles/nearest_points_k.txt.
Each other mode rewrites its own section of profiles/nearest_points.txt and leaves the other."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "profiles" / "nearest_points.txt"
MARK = "==== kernel resources"
N = 1 << 20


def write_section(text, resources):
    old = OUT.read_text() if OUT.exists() else ""
    head, _, tail = old.partition(MARK)
    if resources:
        OUT.write_text(head.rstrip("\n") + ("\n\n" if head.strip() else "") + MARK + text)
    else:
        OUT.write_text(text.rstrip("\n") + "\n" + ("\n" + MARK + tail if tail else ""))


def scenes(names):
    from rvpt_amd import scene
    for name in names:
        tris, mats = {"default": scene.default_scene, "cornell": scene.cornell_scene, "terrain": scene.heightfield_scene}[name]()
        yield name, np.ascontiguousarray(tris), mats


def points(tris, kind, n=N, seed=1):
    """near: a jittered grid of n points through the scene's box; far: n points on a sphere of 10 extents about its centre.  Shuffled: a wave holds points from
    everywhere, as a caller's contact probes would."""
    rng = np.random.RandomState(seed)
    v = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    if kind == "near":
        side = int(np.ceil(n ** (1 / 3) - 1e-9))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
        p = lo + (hi - lo) * (g + rng.uniform(0, 1, g.shape)) / side
    else:
        d = rng.normal(size=(n, 3))
        p = (lo + hi) / 2 + 10.0 * float((hi - lo).max()) * d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.ascontiguousarray(p[rng.permutation(p.shape[0])], dtype=np.float32)


def records_of(pts):
    from rvpt_amd import native
    rec = np.zeros(pts.shape[0], dtype=native.POINT_HIT_DTYPE)
    rec["point"], rec["max_d2"] = pts, np.inf
    return rec


def rate(fn, n, unit, reps=7, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    r = [n / t / 1e6 for t in ts]
    return f"median {statistics.median(r):9.1f}   min {min(r):9.1f}   max {max(r):9.1f}   {unit} (wall clock of the call, n {reps})"


def upload(ctx, name, tris, mats, native):
    if name == "terrain":
        assert ctx.build_scene(tris, mats, "sah") == "sah"
        return "build_scene(sah)"
    nodes, idx = native.build_bvh(tris)
    ctx.upload_scene(nodes, np.ascontiguousarray(tris[idx]), mats)
    return "host build"


def rates(names):
    import torch
    from rvpt_amd import native, scene
    lines = ["point queries: tools/bench_nearest.py rates " + " ".join(names),
             f"{N} records per call, max_d2 = +inf; one MI355X; rates are wall clock around the call (it returns after its stream has finished)", ""]
    done = 0
    for name, tris, mats in scenes(names):
        v = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3)
        ext = float(np.ptp(v, axis=0).max())
        centre = (v.min(axis=0) + v.max(axis=0)) / 2
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
        how = upload(ctx, name, tris, mats, native)
        lines.append(f"== {name}: {tris.shape[0]} triangles, {how}, extent {ext:.2f} ==")
        answers = {}
        for kind in ("near", "far"):
            pts = points(tris, kind)
            rec = records_of(pts)
            dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
            lines.append(f"nearest_bvh2   {kind:5s} host records    {rate(lambda: ctx.closest_points_into(rec), N, 'Mpoints/s')}")
            lines.append(f"nearest_bvh2   {kind:5s} device records  {rate(lambda: ctx.closest_points_into(dev), N, 'Mpoints/s')}")
            got = dev.cpu().numpy().view(native.POINT_HIT_DTYPE).reshape(-1)
            assert got.tobytes() == rec.tobytes(), "host and device records differ"
            answers[kind] = rec
            lines.append(f"{'':20s} mean distance {float(np.sqrt(rec['d2'].astype(np.float64)).mean()) / ext:.3f} extents, regions {np.bincount(rec['region'], minlength=7).tolist()}")
            # yardstick: the ray query's closest hit on the same context, one ray per point towards the scene's centre
            rays = np.zeros(N, dtype=native.RAY_HIT_DTYPE)
            rays["org"], rays["dir"], rays["tmax"] = pts, (centre - pts).astype(np.float32), np.inf
            rdev = torch.from_numpy(rays.view(np.float32).reshape(-1, 12)).to("cuda:0")
            lines.append(f"yardstick: ray query, closest hit, {kind:5s} device records  {rate(lambda: ctx.trace_rays_into(rdev), N, 'Mrays/s')}")
        ctx.close()
        if tris.shape[0] < 100000:  # yardstick: the brute-force kernel, where a brute-force context is practical
            b = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BRUTE)
            nodes, idx = native.build_bvh(tris)
            b.upload_scene(None, np.ascontiguousarray(tris[idx]), mats)
            for kind in ("near", "far"):
                rec = records_of(points(tris, kind))
                dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
                reps = 7 if tris.shape[0] < 1000 else 3
                lines.append(f"nearest_brute  {kind:5s} device records  {rate(lambda: b.closest_points_into(dev), N, 'Mpoints/s', reps=reps, warm=1)}")
                got = dev.cpu().numpy().view(native.POINT_HIT_DTYPE).reshape(-1)
                assert got.tobytes() == answers[kind].tobytes(), "the tree walk and the brute-force kernel differ"
            lines.append(f"{'':20s} the brute-force records equal the tree walk's byte for byte")
            b.close()
        n_cpu = 2000 if tris.shape[0] < 1000 else (200 if tris.shape[0] < 100000 else 4)
        pick = points(tris, "near", n=4096)[:n_cpu]
        t0 = time.perf_counter()
        scene.closest_points(tris, pick)
        dt = time.perf_counter() - t0
        lines.append(f"yardstick: scene.closest_points on this CPU (numpy, brute force), {n_cpu} points: {n_cpu / dt:.1f} points/s")
        lines.append("")
        print("\n".join(lines[done:]), flush=True)
        done = len(lines)
    write_section("\n".join(lines), resources=False)


def rate_g(fn, n, reps=7, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    r = [n / t / 1e9 for t in ts]
    return statistics.median(r), min(r), max(r)


def k_leg(label, names):
    """Gpoints/s (points, that is groups, per second of wall clock around the call) at k = 1, 2, 4, 8, near points, device records"""
    import os
    import torch
    from rvpt_amd import native
    out = ROOT / "profiles" / "nearest_points_k.txt"
    lines = [f"== {label}: tools/bench_nearest.py --k, library {Path(os.environ['RVPT_HIP_LIB']).name if os.environ.get('RVPT_HIP_LIB') else 'in-tree'} ==",
             f"{N} points per call (near: a jittered grid through the scene's box), max_d2 = +inf, device records; Gpoints/s, median (min .. max) of 7 calls"]
    done = 0
    for name, tris, mats in scenes(names):
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
        how = upload(ctx, name, tris, mats, native)
        rec = records_of(points(tris, "near"))
        dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
        lines.append(f"{name}: {tris.shape[0]} triangles, {how}")
        passes = [rate_g(lambda: ctx.closest_points_into(dev), N) for _ in range(3)]  # format 4's own rate, three passes: the figure compared across libraries
        lines.append("  format 4      " + "   ".join(f"{m:7.4f} ({lo:7.4f} .. {hi:7.4f})" for m, lo, hi in passes))
        plain = dev.cpu().numpy().view(native.POINT_HIT_DTYPE).reshape(-1)
        for k in (1, 2, 4, 8):
            groups = np.zeros((N, k), dtype=native.POINT_HIT_DTYPE)
            groups[:, 0] = rec
            gdev = torch.from_numpy(groups.view(np.float32).reshape(-1, 12)).to("cuda:0")
            try:
                m, lo, hi = rate_g(lambda: ctx.closest_points_into(gdev, k=k), N)
            except native.NativeError as e:
                lines.append(f"  k = {k}         this library has no such format ({e})")
                break
            got = gdev.cpu().numpy().view(native.POINT_HIT_DTYPE).reshape(N, k)
            assert np.ascontiguousarray(got[:, 0]).tobytes() == plain.tobytes(), "slot 0 is not format 4's answer"
            assert (got["d2"][:, 1:] >= got["d2"][:, :-1]).all()
            lines.append(f"  k = {k}         {m:7.4f} ({lo:7.4f} .. {hi:7.4f})")
            del gdev
        ctx.close()
        print("\n".join(lines[done:]), flush=True)
        done = len(lines)
    lines.append("")
    with open(out, "a") as f:
        f.write("\n".join(lines) + "\n")


def queries(names, kind):
    import torch
    from rvpt_amd import native
    for name, tris, mats in scenes(names):
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
        upload(ctx, name, tris, mats, native)
        dev = torch.from_numpy(records_of(points(tris, kind)).view(np.float32).reshape(-1, 12)).to("cuda:0")
        for _ in range(8):
            ctx.closest_points_into(dev)
        ctx.close()
        print(f"{name}: 8 queries of {N} device records ({kind}) done")


def resources(parent):
    import importlib.util

    def tables(root, files):
        for k in [k for k in sys.modules if k == "rvpt_amd" or k.startswith("rvpt_amd.")]:
            del sys.modules[k]
        sys.path.insert(0, str(root))
        try:
            spec = importlib.util.spec_from_file_location("kernel_resources", Path(root) / "tools" / "kernel_resources.py")
            m = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(m)
            return m.kernel_resources(files)
        finally:
            sys.path.remove(str(root))

    def table(title, res):
        out = [title, f"  {'kernel':88s} {'vgpr':>5s} {'sgpr':>5s} {'scratch':>8s} {'static_lds':>10s}"]
        for k in sorted(res):
            v = res[k]
            out.append(f"  {k[:88]:88s} {v['vgpr']:5d} {v['sgpr']:5d} {v['scratch_bytes']:8d} {v['static_lds_bytes']:10d}")
        return out

    old_files = sorted(p.name for p in (Path(parent) / "rvpt_amd" / "csrc").glob("*.hip"))
    lines = [" (tools/bench_nearest.py resources <parent tree>; tools/kernel_resources.py: the compiler's own metadata) ====", "",
             "every kernel of every .hip file of the parent commit, there and here (template instances counted one by one):",
             f"  {'file':20s} {'kernels':>8s} {'max vgpr':>9s} {'max sgpr':>9s} {'with scratch':>13s} {'identical':>10s}"]
    same, total = True, 0
    for name in old_files:
        before, after = tables(parent, [name]), tables(ROOT, [name])
        changed = sorted(k for k in set(before) | set(after) if before.get(k) != after.get(k))
        same, total = same and not changed, total + len(after)
        lines.append(f"  {name:20s} {len(after):8d} {max([v['vgpr'] for v in after.values()], default=0):9d} {max([v['sgpr'] for v in after.values()], default=0):9d} "
                     f"{sum(1 for v in after.values() if v['scratch_bytes']):13d} {str(not changed):>10s}" + ("" if not changed else f"   differing: {changed}"))
    lines += ["", f"identical: {same} ({total} kernels: vgpr, sgpr, scratch bytes and static LDS bytes of each)", ""]
    lines += table("the new kernels (rvpt_nearest.hip)", tables(ROOT, ["rvpt_nearest.hip"]))
    text = "\n".join(lines) + "\n"
    print(MARK + text)
    write_section(text, resources=True)
    return same


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rates"
    if mode == "--k":
        k_leg(sys.argv[2] if len(sys.argv) > 2 else "this tree", sys.argv[3:] or ["default", "cornell", "terrain"])
        sys.exit(0)
    if mode == "resources":
        sys.exit(0 if resources(sys.argv[2]) else 1)
    args = sys.argv[2:]
    kind = "far" if "far" in args else "near"
    names = [a for a in args if a not in ("near", "far")] or ["default", "cornell", "terrain"]
    rates(names) if mode == "rates" else queries(names, kind)
