#!/usr/bin/env python3
"""Path queries (rvpt_hip_read with FORMAT_RAY_PATHS; Context.trace_paths_into) measured -> profiles/path_queries.txt.

usage: tools/bench_paths.py [rates] [default_brute default cornell terrain]
       tools/bench_paths.py queries [scene ...]        three device-record queries and three one-frame launches per scene and nothing else: the run to put
                                                       under rocprofv3 (--kernel-trace --stats, or --pmc SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES
                                                       SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY in a run of its own)
       tools/bench_paths.py lanes <counter csv ...>    per kernel of rocprofv3's counter_collection.csv: VALU lane utilisation = SQ_THREAD_CYCLES_VALU /
                                                       (64 SQ_ACTIVE_INST_VALU), as tools/summarize_prof.py has it for the frame kernels, and the waiting share

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
    mode = args.pop(0) if args and args[0] in ("rates", "queries", "lanes") else "rates"
    if mode == "lanes":
        lanes(args)
    elif mode == "queries":
        queries(args or ["cornell", "terrain"])
    else:
        main(args or ["default_brute", "default", "cornell", "terrain"])
