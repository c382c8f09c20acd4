#!/usr/bin/env python3
"""Box queries (rvpt_hip_read with FORMAT_BOX_OVERLAPS / FORMAT_BOX_OVERLAPS_K(k); Context.box_overlaps_into) measured -> profiles/box_overlaps.txt.

usage: tools/bench_boxes.py boxes <label> [default cornell terrain]   on the GPU box: Gboxes/s of 2^20 boxes from device records on each scene — cubes centred on
                                                                      tools/bench_nearest.py's near points (a jittered grid through the scene's box), of three
                                                                      edges: the scene's mean triangle edge, 8 x that, and 1/16 of the extent — at k = 1 and
                                                                      k = 4, with the mean count per box; beside them the same run's format-4 rate on the same
                                                                      centres, and on Cornell box_brute on a brute-force context against box_bvh2 (whose records
                                                                      it must equal byte for byte).
       tools/bench_boxes.py unchanged <label> [scenes]                formats 2 and 4 alone, three passes each, for a library that may not know format 9:
                                                                      with RVPT_HIP_LIB naming the parent commit's library, run alternately with the in-tree
                                                                      one, this shows whether the existing query forms moved.
Both modes print their block and append it to the file BOX_BENCH_OUT names (default profiles/box_overlaps.txt)."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench_nearest as bn  # noqa: E402  (the scenes, the centres, the upload and the timing loop are the point queries')

N = bn.N
OUT = Path(os.environ.get("BOX_BENCH_OUT", ROOT / "profiles" / "box_overlaps.txt"))


def library():
    return Path(os.environ["RVPT_HIP_LIB"]).name if os.environ.get("RVPT_HIP_LIB") else "in-tree"


def emit(lines):
    OUT.parent.mkdir(parents=True, exist_ok=True)
    with open(OUT, "a") as f:
        f.write("\n".join(lines) + "\n")


def mean_edge(tris):
    v = tris.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    return float(np.mean([np.linalg.norm(v[:, i] - v[:, (i + 1) % 3], axis=1).mean() for i in range(3)]))


def groups_of(centres, edge, k):
    from rvpt_amd import native
    rec = np.zeros((centres.shape[0], k), dtype=native.BOX_OVERLAP_DTYPE)
    half = np.float32(edge / 2)
    rec["lo"][:, 0], rec["hi"][:, 0] = centres - half, centres + half
    return rec


def fmt(triple):
    m, lo, hi = triple
    return f"{m:7.4f} ({lo:7.4f} .. {hi:7.4f})"


def boxes(label, names):
    import torch
    from rvpt_amd import native
    lines = [f"== {label}: tools/bench_boxes.py boxes, library {library()} ==",
             f"{N} boxes per call from device records, prim_from 0; Gboxes/s (boxes per second of wall clock around the call, which returns after its stream has "
             "finished), median (min .. max) of 7 calls after 2 warm-up calls; one MI355X"]
    done = 0
    for name, tris, mats in bn.scenes(names):
        v = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3)
        ext, edge = float(np.ptp(v, axis=0).max()), mean_edge(tris)
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
        how = bn.upload(ctx, name, tris, mats, native)
        centres = bn.points(tris, "near")
        lines.append(f"{name}: {tris.shape[0]} triangles, {how}, extent {ext:.3f}, mean triangle edge {edge:.4f}")
        pdev = torch.from_numpy(bn.records_of(centres).view(np.float32).reshape(-1, 12)).to("cuda:0")
        lines.append(f"  yardstick: format 4 (nearest point) on the same centres   {fmt(bn.rate_g(lambda: ctx.closest_points_into(pdev), N))} Gpoints/s")
        del pdev
        brute = None
        if name == "cornell":
            brute = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BRUTE)
            nodes, idx = native.build_bvh(tris)
            brute.upload_scene(None, np.ascontiguousarray(tris[idx]), mats)
        for what, e in (("mean triangle edge", edge), ("8 x mean triangle edge", 8 * edge), ("extent / 16", ext / 16)):
            for k in (1, 4):
                rec = groups_of(centres, e, k)
                dev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
                r = bn.rate_g(lambda: ctx.box_overlaps_into(dev, k=k), N)
                got = dev.cpu().numpy().view(native.BOX_OVERLAP_DTYPE).reshape(N, k)
                count, numbers = native.box_overlap_lists(got, k)
                full = float((count > numbers.shape[1]).mean())
                lines.append(f"  box_bvh2  edge {e:9.4f} ({what:22s}) k = {k}   {fmt(r)} Gboxes/s   mean count {count.mean():9.2f}, max {int(count.max())}, "
                             f"{100 * full:5.1f} % of the boxes hold more than the {numbers.shape[1]} listed")
                if brute is not None:
                    bdev = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
                    rb = bn.rate_g(lambda: brute.box_overlaps_into(bdev, k=k), N, reps=3, warm=1)
                    assert bdev.cpu().numpy().tobytes() == got.view(np.float32).tobytes(), "the tree walk and the brute-force kernel differ"
                    lines.append(f"  box_brute edge {e:9.4f} ({what:22s}) k = {k}   {fmt(rb)} Gboxes/s (3 calls)   the same bytes; box_bvh2 is {r[0] / rb[0]:.1f} x")
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


def unchanged(label, names):
    import torch
    from rvpt_amd import native
    lines = [f"== {label}: tools/bench_boxes.py unchanged, library {library()} ==",
             f"{N} records per call from device records; format 2: closest hit of rays from the near points towards the scene's centre, Grays/s; format 4: the near "
             "points, Gpoints/s; three passes of median (min .. max) of 7 calls"]
    done = 0
    for name, tris, mats in bn.scenes(names):
        v = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3)
        centre = (v.min(axis=0) + v.max(axis=0)) / 2
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
        how = bn.upload(ctx, name, tris, mats, native)
        pts = bn.points(tris, "near")
        rays = np.zeros(N, dtype=native.RAY_HIT_DTYPE)
        rays["org"], rays["dir"], rays["tmax"] = pts, (centre - pts).astype(np.float32), np.inf
        rdev = torch.from_numpy(rays.view(np.float32).reshape(-1, 12)).to("cuda:0")
        pdev = torch.from_numpy(bn.records_of(pts).view(np.float32).reshape(-1, 12)).to("cuda:0")
        lines.append(f"{name}: {tris.shape[0]} triangles, {how}")
        lines.append("  format 2      " + "   ".join(fmt(bn.rate_g(lambda: ctx.trace_rays_into(rdev), N)) for _ in range(3)))
        lines.append("  format 4      " + "   ".join(fmt(bn.rate_g(lambda: ctx.closest_points_into(pdev), N)) for _ in range(3)))
        ctx.close()
        print("\n".join(lines[done:]), flush=True)
        done = len(lines)
    lines.append("")
    emit(lines)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "boxes"
    label = sys.argv[2] if len(sys.argv) > 2 else "this tree"
    names = sys.argv[3:] or ["default", "cornell", "terrain"]
    if mode not in ("boxes", "unchanged"):
        sys.exit(__doc__)
    boxes(label, names) if mode == "boxes" else unchanged(label, names)
