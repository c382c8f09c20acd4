#!/usr/bin/env python3
"""Sphere sweeps (rvpt_hip_read with FORMAT_SPHERE_SWEEPS; Context.sweep_spheres_into) measured -> profiles/sphere_sweeps.txt.

usage: tools/bench_sweeps.py sweeps <label> [default cornell terrain]   on the GPU box: Gsweeps/s of 2^20 sweeps from device records on each scene — centres at
                                                                        tools/bench_nearest.py's near points (a jittered grid through the scene's box) moving
                                                                        towards the scene's centre, tmax = inf, with radius 0, one and eight mean triangle
                                                                        edges — with the share of hits and of initial overlaps; beside them the same run's
                                                                        format-2 rate on the same rays (the sweep of radius 0) and format-4 rate on the origins,
                                                                        and on Cornell sweep_brute on a brute-force context against sweep_bvh2 (whose records
                                                                        it must equal byte for byte).
       tools/bench_sweeps.py unchanged <label> [scenes]                 formats 2 and 4 alone, three passes each, for a library that may not know format 10
                                                                        (tools/bench_boxes.py's mode): with RVPT_HIP_LIB naming the parent commit's library, run
                                                                        alternately with the in-tree one, this shows whether the existing query forms moved.
Both modes print their block and append it to the file SWEEP_BENCH_OUT names (default profiles/sphere_sweeps.txt)."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
OUT = Path(os.environ.get("SWEEP_BENCH_OUT", ROOT / "profiles" / "sphere_sweeps.txt"))
os.environ.setdefault("BOX_BENCH_OUT", str(OUT))  # (bench_boxes' `unchanged` block goes to this form's file)
import bench_boxes as bb  # noqa: E402  (mean_edge, fmt, library and the `unchanged` mode are the box queries')
import bench_nearest as bn  # noqa: E402  (the scenes, the centres, the upload and the timing loop are the point queries')

N = bn.N


def emit(lines):
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


def sweeps(label, names):
    import torch
    from rvpt_amd import native
    lines = [f"== {label}: tools/bench_sweeps.py sweeps, library {bb.library()} ==",
             f"{N} sweeps per call from device records, tmax inf; Gsweeps/s (records per second of wall clock around the call, which returns after its stream has "
             "finished), median (min .. max) of 7 calls after 2 warm-up calls; one MI355X"]
    done = 0
    for name, tris, mats in bn.scenes(names):
        v = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3)
        centre = (v.min(axis=0) + v.max(axis=0)) / 2
        ext, edge = float(np.ptp(v, axis=0).max()), bb.mean_edge(tris)
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
        how = bn.upload(ctx, name, tris, mats, native)
        pts = bn.points(tris, "near")
        dirs = (centre - pts).astype(np.float32)
        lines.append(f"{name}: {tris.shape[0]} triangles, {how}, extent {ext:.3f}, mean triangle edge {edge:.4f}")
        rays = np.zeros(N, dtype=native.RAY_HIT_DTYPE)
        rays["org"], rays["dir"], rays["tmax"] = pts, dirs, np.inf
        rdev = torch.from_numpy(rays.view(np.float32).reshape(-1, 12)).to("cuda:0")
        pdev = torch.from_numpy(bn.records_of(pts).view(np.float32).reshape(-1, 12)).to("cuda:0")
        lines.append(f"  yardstick: format 2 (closest hit) on the same rays          {bb.fmt(bn.rate_g(lambda: ctx.trace_rays_into(rdev), N))} Grays/s")
        lines.append(f"  yardstick: format 4 (nearest point) on the origins          {bb.fmt(bn.rate_g(lambda: ctx.closest_points_into(pdev), N))} Gpoints/s")
        del rdev, pdev
        brute = None
        if name == "cornell":
            brute = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BRUTE)
            nodes, idx = native.build_bvh(tris)
            brute.upload_scene(None, np.ascontiguousarray(tris[idx]), mats)
        for what, r in (("radius 0", 0.0), ("one mean triangle edge", edge), ("8 x mean triangle edge", 8 * edge)):
            rec = np.zeros(N, dtype=native.SPHERE_SWEEP_DTYPE)
            rec["org"], rec["dir"], rec["radius"], rec["tmax"] = pts, dirs, np.float32(r), np.inf
            dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
            rate = bn.rate_g(lambda: ctx.sweep_spheres_into(dev), N)
            got = dev.cpu().numpy().view(native.SPHERE_SWEEP_DTYPE).reshape(N)
            hit = got["prim"] != native.NO_PRIM
            lines.append(f"  sweep_bvh2  radius {r:9.4f} ({what:22s})   {bb.fmt(rate)} Gsweeps/s   {100 * hit.mean():5.1f} % hits, "
                         f"{100 * (hit & (got['t'] == 0)).mean():5.1f} % initial overlaps")
            if brute is not None:
                bdev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
                rb = bn.rate_g(lambda: brute.sweep_spheres_into(bdev), N, reps=3, warm=1)
                same = bdev.cpu().numpy().view(native.SPHERE_SWEEP_DTYPE).reshape(N)
                stored_t = same["t"].tobytes() == got["t"].tobytes()  # (the brute-force context numbers the host builder's leaf order: t is the common part)
                lines.append(f"  sweep_brute radius {r:9.4f} ({what:22s})   {bb.fmt(rb)} Gsweeps/s (3 calls)   t {'the same bytes' if stored_t else 'DIFFERS'}; "
                             f"sweep_bvh2 is {rate[0] / rb[0]:.1f} x")
                del bdev
            del dev
            print("\n".join(lines[done:]), flush=True)
            done = len(lines)
        ctx.close()
        if brute is not None:
            brute.close()
        lines.append("")
        print("\n".join(lines[done:]), flush=True)
        done = len(lines)
    emit(lines)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "sweeps"
    label = sys.argv[2] if len(sys.argv) > 2 else "this tree"
    names = sys.argv[3:] or ["default", "cornell", "terrain"]
    if mode not in ("sweeps", "unchanged"):
        sys.exit(__doc__)
    sweeps(label, names) if mode == "sweeps" else bb.unchanged(label, names)
