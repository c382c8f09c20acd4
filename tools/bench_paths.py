#!/usr/bin/env python3
"""Path queries (rvpt_hip_read with FORMAT_RAY_PATHS; Context.trace_paths_into) measured -> profiles/path_queries.txt.

usage: tools/bench_paths.py [rates] [default_brute default cornell terrain]
       tools/bench_paths.py queries [scene ...]        three device-record queries and three one-frame launches per scene and nothing else: the run to put
                                                       under rocprofv3 (--kernel-trace --stats, or --pmc SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES
                                                       SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY in a run of its own)
       tools/bench_paths.py lanes <counter csv ...>    per kernel of rocprofv3's counter_collection.csv: VALU lane utilisation = SQ_THREAD_CYCLES_VALU /
                                                       (64 SQ_ACTIVE_INST_VALU), as tools/summarize_prof.py has it for the frame kernels, and the waiting share

       tools/bench_paths.py modes [format3] [cornell terrain]   the integrators per call (RVPT_HIP_FORMAT_RAY_PATHS_MODE): format 3 and every mode 0 .. 8 in one
                                                       run, from device records; `format3` measures format 3 alone — the leg to run on the parent commit's
                                                       library (RVPT_HIP_LIB=<its librvpt_hip.so>) in the same session, before and after.  Prints the section
                                                       profiles/path_modes.txt keeps
       tools/bench_paths.py resources <parent tree>    tools/kernel_resources.py on every .hip file of the parent tree and of this one: are the figures of the
                                                       kernels the parent has unchanged, and what do the new instances of rvpt_paths.hip take

rates, on the GPU box.  Per scene: the 1920 x 1080 jittered pinhole camera rays of frame 0 with the RNG states a frame's pixels continue from (made here in numpy: the
frame's own rays to rounding, which is all a rate needs), max_bounces 8, as 2 M records — paths/s and segments/s from device records and from host records,
wall clock around the call (it returns after its stream has finished).  Beside them, taken in the same run and alternating with the queries: the same context's
one-frame launch of that frame (max_bounces 8, aa 1), its segments from RVPT_HIP_COUNT_SEGMENTS and its kernel time from RVPT_HIP_TIMING.  The yardstick is that
launch, never an earlier run of the query."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "profiles" / "path_queries.txt"
W, H = 1920, 1080
BOUNCES = 8
REPS, WARM = 7, 2


def scenes(names):
    from rvpt_amd import Camera, native, scene
    for name in names:
        c = Camera(W / H)
        if name.startswith("default"):
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


def frame_records(cam, frame):
    """pixel (x, y)'s jittered pinhole ray of frame `frame` (compute_pass.comp:151-156, camera.glsl:29-51) and the RNG state after its two jitter draws"""
    from rvpt_amd import native
    from rvpt_amd.renderer import wang_hash
    cam = np.asarray(cam, dtype=np.float32)
    m = cam[:16].reshape(4, 4).T.astype(np.float64)
    state = wang_hash(np.arange(W * H, dtype=np.uint32)) + np.uint32(frame)
    draws = []
    for _ in range(2):
        state ^= state << np.uint32(13)
        state ^= state >> np.uint32(17)
        state ^= state << np.uint32(5)
        draws.append(state.astype(np.float32) * np.float32(2.3283064365386962890625e-10))
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    cx = (x.reshape(-1) + draws[0]) * np.float32(1.0 / W)
    cy = np.float32(1.0) - (y.reshape(-1) + draws[1]) * np.float32(1.0 / H)
    u, v, w = float(cam[16]) * (2.0 * cx.astype(np.float64) - 1.0), 2.0 * cy.astype(np.float64) - 1.0, 1.0 / np.tan(0.5 * float(cam[17]))
    d = u[:, None] * m[:3, 0] + v[:, None] * m[:3, 1] + w * m[:3, 2]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rec = np.zeros(W * H, dtype=native.RAY_PATH_DTYPE)
    rec["org"], rec["dir"], rec["seed"], rec["max_bounces"] = m[:3, 3].astype(np.float32), d.astype(np.float32), state, BOUNCES
    return rec


def spread(values, unit):
    return f"median {statistics.median(values):9.1f}   min {min(values):9.1f}   max {max(values):9.1f}   {unit} (n {len(values)})"


def main(names):
    import torch
    from rvpt_amd import RenderSettings, native
    lines = ["path queries: tools/bench_paths.py " + " ".join(names),
             f"{W} x {H} jittered pinhole camera rays of frame 0 = {W * H} records per call, max_bounces {BOUNCES}; one MI355X", "query rates: wall clock around the call (it returns after its stream has finished); "
             "frame launch: RVPT_HIP_TIMING's kernel time of a one-frame launch of the same frame on the same context, segments from RVPT_HIP_COUNT_SEGMENTS",
             f"{WARM} warm-up rounds, then {REPS} rounds of (device-record query, host-record query, frame launch), alternating", ""]
    for name, tris, mats, nodes, cam in scenes(names):
        brute = name.endswith("_brute")
        ctx = native.Context(W, H, 0, 0, 1, (native.TRAVERSAL_BRUTE if brute else native.TRAVERSAL_BVH) | native.COUNT_SEGMENTS | native.TIMING)
        ctx.upload_scene(None if brute else nodes, tris, mats)
        rec = frame_records(cam, 0)
        dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
        settings = RenderSettings(max_bounces=BOUNCES, aa=1, current_frame=0).pack()
        t_dev, t_host, t_frame, frame_segments = [], [], [], 0
        for k in range(WARM + REPS):
            t0 = time.perf_counter()
            ctx.trace_paths_into(dev)
            t1 = time.perf_counter()
            ctx.trace_paths_into(rec)
            t2 = time.perf_counter()
            s0 = ctx.stats()[0]
            ctx.set_frame(settings, cam)
            ctx.dispatch()
            ctx.wait()
            frame_ms, frame_segments = ctx.timing()[0], ctx.stats()[0] - s0
            if k >= WARM:
                t_dev.append(t1 - t0), t_host.append(t2 - t1), t_frame.append(frame_ms * 1e-3)
        got = dev.cpu().numpy().view(native.RAY_PATH_DTYPE).reshape(-1)
        assert got.tobytes() == rec.tobytes(), "host and device records differ"
        segments = int(rec["segments"].sum(dtype=np.uint64))
        hist = np.bincount(rec["segments"], minlength=BOUNCES + 1)[:BOUNCES + 1]
        lines.append(f"== {name}: {tris.shape[0]} triangles, {'brute force' if brute else f'BVH, {nodes.shape[0]} nodes'}; frame kernel variant {ctx.launch_info()[2]} ==")
        lines.append(f"query: {segments} segments in {W * H} paths ({segments / (W * H):.2f} per path; paths by segments 0..{BOUNCES}: {hist.tolist()}); the frame launch counts {frame_segments}")
        for what, ts in (("device records", t_dev), ("host records", t_host)):
            lines.append(f"  {what:15s} {spread([W * H / t / 1e6 for t in ts], 'Mpaths/s   ')}")
            lines.append(f"  {'':15s} {spread([segments / t / 1e6 for t in ts], 'Msegments/s')}")
        frame_rates = [frame_segments / t / 1e6 for t in t_frame]
        lines.append(f"  {'frame launch':15s} {spread(frame_rates, 'Msegments/s')}   kernel {statistics.median(t_frame) * 1e3:.3f} ms")
        lines.append(f"  device-record query / frame launch, segment rates (medians): {statistics.median([segments / t / 1e6 for t in t_dev]) / statistics.median(frame_rates):.3f}")
        lines.append("")
        ctx.close()
    text = "\n".join(lines)
    print(text)
    OUT.write_text(text)


def queries(names):
    import torch
    from rvpt_amd import RenderSettings, native
    for name, tris, mats, nodes, cam in scenes(names):
        brute = name.endswith("_brute")
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE if brute else native.TRAVERSAL_BVH)
        ctx.upload_scene(None if brute else nodes, tris, mats)
        dev = torch.from_numpy(frame_records(cam, 0).view(np.float32).reshape(-1, 12)).to("cuda:0")
        for _ in range(3):
            ctx.trace_paths_into(dev)
            ctx.set_frame(RenderSettings(max_bounces=BOUNCES, aa=1, current_frame=0).pack(), cam)
            ctx.dispatch()
            ctx.wait()
        ctx.close()
        print(f"{name}: 3 queries of {W * H} device records and 3 one-frame launches done")


def modes(args):
    """Per scene (Cornell as uploaded with the host-built tree; the 1 M-triangle terrain after build_scene("sah")): the 2 M camera rays of a 1080p frame as
    device records, budget 8, asked with format 3 and with every mode 0 .. 8, alternating within each round; wall clock of the call, median of REPS rounds"""
    import os
    import torch
    from rvpt_amd import native, scene
    format3_only = bool(args) and args[0] == "format3"
    names = (args[1:] if format3_only else args) or ["cornell", "terrain"]
    forms = [("format 3", None)] + ([] if format3_only else [(f"mode {m}", m) for m in range(9)])
    lib = os.environ.get("RVPT_HIP_LIB")
    lines = ["path queries by integrator: tools/bench_paths.py modes " + " ".join(args) + (f"   (library: {Path(lib).name})" if lib else "   (library: this tree's)"),
             f"{W} x {H} jittered pinhole camera rays of frame 0 = {W * H} device records per call, max_bounces {BOUNCES}; one MI355X; wall clock around the call",
             f"{WARM} warm-up rounds, then {REPS} rounds, every form once per round in turn; per form: median, min and max over the rounds", ""]
    for name in names:
        c = native_camera(name)
        if name == "cornell":
            tris, mats = scene.cornell_scene()
            nodes, idx = native.build_bvh(tris)
            ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
            ctx.upload_scene(nodes, tris[idx], mats)
            how = f"host-built tree, {nodes.shape[0]} nodes"
        else:
            tris, mats = scene.heightfield_scene()
            ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
            how = f"build_scene(\"{ctx.build_scene(tris, mats, 'sah')}\")"
        rec = frame_records(c, 0)
        dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
        times = {what: [] for what, _ in forms}
        for k in range(WARM + REPS):
            for what, mode in forms:
                t0 = time.perf_counter()
                ctx.trace_paths_into(dev) if mode is None else ctx.trace_paths_into(dev, mode=mode)
                if k >= WARM:
                    times[what].append(time.perf_counter() - t0)
        lines.append(f"== {name}: {tris.shape[0]} triangles, {how} ==")
        lines.append(f"  {'form':9s} {'segments':>10s} {'/record':>8s}   {'Mrecords/s: median':>18s} {'min':>8s} {'max':>8s}   {'Gsegments/s: median':>19s} {'min':>7s} {'max':>7s}   {'ms: median':>10s}")
        for what, mode in forms:
            ctx.trace_paths_into(dev) if mode is None else ctx.trace_paths_into(dev, mode=mode)
            segments = int(dev.cpu().numpy().view(native.RAY_PATH_DTYPE).reshape(-1)["segments"].sum(dtype=np.uint64))
            rr = [W * H / t / 1e6 for t in times[what]]
            sr = [segments / t / 1e9 for t in times[what]]
            lines.append(f"  {what:9s} {segments:10d} {segments / (W * H):8.2f}   {statistics.median(rr):18.1f} {min(rr):8.1f} {max(rr):8.1f}   {statistics.median(sr):19.3f} {min(sr):7.3f} {max(sr):7.3f}"
                         f"   {statistics.median(times[what]) * 1e3:10.3f}")
        lines.append("")
        ctx.close()
    print("\n".join(lines))


def native_camera(name):
    from rvpt_amd import Camera
    c = Camera(W / H)
    if name == "cornell":
        c.translation = np.array([0.0, 2.0, -1.9])
    else:
        c.translation = np.array([0.0, 2.5, -5.0])
        c.rotation = np.array([0.0, 25.0, 0.0])
    return c.get_data()


def resources(parent):
    """The compiler's own figures (tools/kernel_resources.py) for every .hip file of the parent tree, there and here, and for rvpt_paths.hip's instances here"""
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
        out = [title, f"  {'kernel':72s} {'vgpr':>5s} {'sgpr':>5s} {'scratch':>8s} {'static_lds':>10s} {'waves/SIMD by vgpr':>19s}"]
        for k in sorted(res):
            v = res[k]
            out.append(f"  {k[:72]:72s} {v['vgpr']:5d} {v['sgpr']:5d} {v['scratch_bytes']:8d} {v['static_lds_bytes']:10d} {v['waves_per_simd_by_vgpr']:19d}")
        return out

    lean = lambda k: k.replace("<0>", "")  # the parent's path kernels are this tree's LEAN instances (template argument 0)
    lines = ["==== kernel resources (tools/bench_paths.py resources <parent tree>; tools/kernel_resources.py: the compiler's own metadata) ====", "",
             "every kernel of every .hip file of the parent commit, there and here (template instances counted one by one; rvpt_paths.hip: the parent's three kernels",
             "against this tree's LEAN instances path_*<0>, the instances beyond them listed below):",
             f"  {'file':20s} {'kernels':>8s} {'max vgpr':>9s} {'max sgpr':>9s} {'with scratch':>13s} {'identical':>10s}"]
    same, total = True, 0
    for name in sorted(p.name for p in (Path(parent) / "rvpt_amd" / "csrc").glob("*.hip")):
        before, after = tables(parent, [name]), {lean(k): v for k, v in tables(ROOT, [name]).items()}
        after = {k: v for k, v in after.items() if k in before} if name == "rvpt_paths.hip" else after
        changed = sorted(k for k in set(before) | set(after) if before.get(k) != after.get(k))
        same, total = same and not changed, total + len(after)
        lines.append(f"  {name:20s} {len(after):8d} {max([v['vgpr'] for v in after.values()], default=0):9d} {max([v['sgpr'] for v in after.values()], default=0):9d} "
                     f"{sum(1 for v in after.values() if v['scratch_bytes']):13d} {str(not changed):>10s}" + ("" if not changed else f"   differing: {changed}"))
    lines += ["", f"identical: {same} ({total} kernels: vgpr, sgpr, scratch bytes and static LDS bytes of each)", ""]
    lines += table("rvpt_paths.hip on the parent commit", tables(parent, ["rvpt_paths.hip"])) + [""]
    lines += table("rvpt_paths.hip here: <0> LEAN (format 3 and mode 9), <1> HIT_ONLY (modes 0 .. 4), <2> CONTINUING (modes 5 .. 8)", tables(ROOT, ["rvpt_paths.hip"]))
    print("\n".join(lines))
    return same


def lanes(files):
    import csv
    from collections import defaultdict
    for f in files:
        total = defaultdict(lambda: defaultdict(float))
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                total[row["Kernel_Name"].split("(")[0]][row["Counter_Name"]] += float(row["Counter_Value"])
        print(f"== {f} ==")
        for kernel, c in sorted(total.items()):
            if "path_" not in kernel and "trace_" not in kernel:
                continue
            out = [f"{kernel[:60]:60s}"]
            if c.get("SQ_ACTIVE_INST_VALU"):
                out.append(f"VALU lane utilisation {c['SQ_THREAD_CYCLES_VALU'] / (64.0 * c['SQ_ACTIVE_INST_VALU']):.3f}")
            if c.get("SQ_WAVE_CYCLES"):
                out.append(f"of wave cycles: waiting at s_waitcnt {c.get('SQ_WAIT_INST_ANY', 0.0) / c['SQ_WAVE_CYCLES']:.3f}, issuing {c.get('SQ_ACTIVE_INST_ANY', 0.0) / c['SQ_WAVE_CYCLES']:.3f}")
            print("   ".join(out))


if __name__ == "__main__":
    args = sys.argv[1:]
    mode = args.pop(0) if args and args[0] in ("rates", "queries", "lanes", "modes", "resources") else "rates"
    if mode == "modes":
        modes(args)
    elif mode == "resources":
        sys.exit(0 if resources(args[0]) else 1)
    elif mode == "lanes":
        lanes(args)
    elif mode == "queries":
        queries(args or ["cornell", "terrain"])
    else:
        main(args or ["default_brute", "default", "cornell", "terrain"])
