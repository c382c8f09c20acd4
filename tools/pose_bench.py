#!/usr/bin/env python3
"""Run on the GPU box: what the POSE UPDATE of rvpt_hip_upload_scene (Context.pose_parts) costs on the 1 M-triangle terrain (BVH context, 1920x1080), after
build_scene(method="sah") and after an ordinary upload, beside the yardsticks of the same run — the plain update form from a host array and from a device
tensor, and the sparse update of the same 1 % block.  Candidates: one part of 1 % of the triangles, 100 parts of 1 % each, one part holding everything.  All
six alternate inside one loop (wall clock of the call, median of 20 after 3 warm-up rounds).  Then what traversal pays on a posed, refitted tree against a
tree rebuilt for that pose, for a small rotation of one part and for a part carried across the scene.  -> stdout (profiles/pose_update.txt)
Exits non-zero unless the whole-mesh pose costs less than the plain update from a host array in the same run: the plain form is bound by a 48 MB copy that
the pose form does not make.
usage: tools/pose_bench.py [all|updates|guard]     (updates: a device build and a few pose updates of each kind, nothing else — the run to put under
rocprofv3 --kernel-trace --stats; guard: the GUARDED POSE UPDATE (Context.pose_parts(rebuild_above=)) alone -> stdout (profiles/guarded_pose.txt): what the
guard adds to a plain pose of a 1 % part, both alternating in one loop on one context; what a guarded pose that rebuilds costs, per builder; and the two motions
of the traversal table under a limit of 1.1 — the ratio each reports, what was decided, and the one-frame rate afterwards beside the refitted and the freshly
built rates.  Nothing there is a pass/fail bar.)"""
import math, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rvpt_amd import Camera, RenderSettings, native, scene  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
W, H = 1920, 1080


def spread(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms   min {min(xs) * 1e3:9.3f}   max {max(xs) * 1e3:9.3f}   n {len(xs)}"


def rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def about(centre, rot):
    c = np.asarray(centre, dtype=np.float64)
    return np.concatenate([rot, (c - rot @ c).reshape(3, 1)], axis=1)


def centroid(tris, first, count):
    return tris[first:first + count].reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64).mean(axis=0)


def move_lists(tris, flip):
    """the three candidate lists for one of two alternating poses (flip 0 / 1): one part of 1 %, 100 parts of 1 % each, one part of everything"""
    n = tris.shape[0]
    k = n // 100
    angle = 0.02 if flip else -0.02
    one = scene.part_moves([(n // 2, k, about(centroid(tris, n // 2, k), rotation_y(angle)))])
    hundred = scene.part_moves([(p * k, k if p < 99 else n - 99 * k, about(centroid(tris, p * k, k), rotation_y(angle * (1 + p % 3)))) for p in range(100)])
    whole = scene.part_moves([(0, n, about(centroid(tris, 0, n), rotation_y(angle)))])
    return {"pose, 1 part of 1 %": one, "pose, 100 parts of 1 % each": hundred, "pose, 1 part of everything": whole}


def frame_rate(ctx, cam, frames=24, reps=5):
    """Msamples/s of one-frame launches (a moving mesh leaves nothing to batch), wall clock over `frames` frames"""
    out = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        for f in range(frames):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ctx.wait()
        if rep:
            out.append(W * H * frames / (time.perf_counter() - t0) / 1e6)
    return out


def updates_section(ctx, tris, label):
    """`tris`: the triangles in the order the update forms take on ctx"""
    import torch
    n = tris.shape[0]
    k = n // 100
    ext = float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
    poses = [scene.wobble(tris, 0.5 + 0.9 * j, 0.02 * ext) for j in range(2)]
    dev_poses = [torch.from_numpy(p).to("cuda:0") for p in poses]
    block = np.arange(n // 2, n // 2 + k)
    rows = [np.ascontiguousarray(p[block]) for p in poses]
    lists = [move_lists(tris, flip) for flip in (0, 1)]
    variants = {"plain update, host numpy array": lambda j: ctx.update_triangles(poses[j]),
                "plain update, torch tensor on device": lambda j: ctx.update_triangles(dev_poses[j]),
                "sparse update, the 1 % block, host arrays": lambda j: ctx.update_triangles(rows[j], indices=block)}
    for name in lists[0]:
        variants[name] = (lambda nm: lambda j: ctx.pose_parts(lists[j][nm]))(name)
    times = {name: [] for name in variants}
    for it in range(23):  # the candidates and the yardsticks alternate: whatever drifts, drifts for all of them
        for name, fn in variants.items():
            t0 = time.perf_counter()
            fn(it % 2)
            if it >= 3:
                times[name].append(time.perf_counter() - t0)
    print(f"\n== {label}: {n} triangles, parts of {k} (wall clock of the call, host call to return; alternating in one loop) ==")
    for name, ts in times.items():
        print(f"{name:44s} {spread(ts)}")
    med = {name: statistics.median(ts) for name, ts in times.items()}
    host, dev, whole = med["plain update, host numpy array"], med["plain update, torch tensor on device"], med["pose, 1 part of everything"]
    ok = whole < host
    print(f"whole-mesh pose / plain update from a host array = {whole / host:.3f} -> {'ok' if ok else 'NOT QUICKER'};   whole-mesh pose / plain update from device memory = {whole / dev:.2f}")
    print(f"1 % pose / sparse update of the same block from host arrays = {med['pose, 1 part of 1 %'] / med['sparse update, the 1 % block, host arrays']:.2f}")
    return ok


tris0, mats = scene.heightfield_scene()
n = tris0.shape[0]
ext = float(np.ptp(tris0.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
c = Camera(W / H)
c.translation = np.array([0.0, 2.5, -5.0])
c.rotation = np.array([0.0, 25.0, 0.0])
cam = c.get_data()
print(f"scene: {n} triangles, extent {ext:.2f}")
ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
ctx.build_scene(tris0, mats, method="sah")

if what == "updates":
    lists = [move_lists(tris0, flip) for flip in (0, 1)]
    for name in lists[0]:
        for j in range(6):
            ctx.pose_parts(lists[j % 2][name])
    ctx.close()
    print("18 pose updates done: 6 of one 1 % part, 6 of 100 parts, 6 of the whole mesh")
    sys.exit(0)



def guard_section(ctx):
    k = n // 100
    lists = [move_lists(tris0, flip)["pose, 1 part of 1 %"] for flip in (0, 1)]
    variants = {"plain pose, 1 part of 1 %": lambda j: ctx.pose_parts(lists[j]),
                "guarded pose, report only, the same part": lambda j: ctx.pose_parts(lists[j], rebuild_above=math.inf),
                "guarded pose, limit 1.1 (never reached), the same part": lambda j: ctx.pose_parts(lists[j], rebuild_above=1.1)}
    times = {name: [] for name in variants}
    for it in range(23):  # the candidate and its yardstick alternate: whatever drifts, drifts for both
        for name, fn in variants.items():
            t0 = time.perf_counter()
            rep = fn(it % 2)
            if it >= 3:
                times[name].append(time.perf_counter() - t0)
            assert rep is None or not rep.rebuilt
    print(f"\n== the guard's cost: {n} triangles, one part of {k}, SAH device build (wall clock of the call; alternating in one loop on one context) ==")
    for name, ts in times.items():
        print(f"{name:56s} {spread(ts)}")
    med = {name: statistics.median(ts) for name, ts in times.items()}
    plain = med["plain pose, 1 part of 1 %"]
    print(f"guarded (report only) - plain = {(med['guarded pose, report only, the same part'] - plain) * 1e3:.3f} ms;   guarded / plain = {med['guarded pose, report only, the same part'] / plain:.2f}")

    first, count = n // 2, n // 10
    centre = centroid(tris0, first, count)
    turned = [(first, count, about(centre, rotation_y(np.radians(2.0))))]
    carried = [(first, count, scene.part_move(0, 1, translation=(0.5 * ext, 0.1 * ext, 0.0))["m"].reshape(3, 4))]
    home = [(first, count, np.eye(3, 4))]
    print("\n== a guarded pose that rebuilds (limit 1.0; the part carried across the scene and brought home in turn, each on the tree built for the other; wall clock of the call) ==")
    for method in ("lbvh", "ploc", "sah"):
        built = ctx.build_scene(tris0, mats, method=method)
        ts, kept = [], 0
        for it in range(7):
            t0 = time.perf_counter()
            rep = ctx.pose_parts(carried if it % 2 == 0 else home, rebuild_above=1.0)
            dt = time.perf_counter() - t0
            if rep.rebuilt and it >= 1:
                ts.append(dt)
            kept += not rep.rebuilt
        print(f"{method:5s} (the scene holds: {built:4s}) " + (spread(ts) if ts else "never rebuilt") + f"   calls that refitted: {kept} of 7")

    print("\n== the two motions under a limit of 1.1 (SAH device build, one-frame launches at 1080p, Msamples/s, median of 5 x 24 frames) ==")
    ctx.build_scene(tris0, mats, method="sah")
    print(f"rest pose, built tree                                        {statistics.median(frame_rate(ctx, cam)):8.0f}")
    for name, moves in (("a rotation of one part (10 % of the mesh) by 2 degrees", turned), ("the same part carried across the scene", carried)):
        ctx.build_scene(tris0, mats, method="sah")
        ctx.pose_parts(moves)
        refitted = statistics.median(frame_rate(ctx, cam))
        ctx.build_scene(tris0, mats, method="sah")
        rep = ctx.pose_parts(moves, rebuild_above=1.1)
        guarded = statistics.median(frame_rate(ctx, cam))
        ctx.build_scene(scene.pose_parts(tris0, moves), mats, method="sah")
        fresh = statistics.median(frame_rate(ctx, cam))
        print(f"{name:56s} ratio {rep.ratio:8.4f} -> {'rebuilt (' + rep.tree + ')' if rep.rebuilt else 'refitted':14s}   afterwards {guarded:8.0f}   plain pose, refitted {refitted:8.0f}   "
              f"fresh build {fresh:8.0f}   afterwards / fresh = {guarded / fresh:.3f}")


if what == "guard":
    guard_section(ctx)
    ctx.close()
    sys.exit(0)

ok = updates_section(ctx, tris0, "after build_scene(method='sah'), ranges in the caller's order")
nodes, idx = native.build_bvh(tris0)
tris = tris0[idx]
ctx.upload_scene(nodes, tris, mats)
ok = updates_section(ctx, tris, "after an ordinary upload of rvpt_bvh_build's tree, ranges in leaf order") and ok

print("\n== what refitting a pose costs in traversal: the posed scene on the refitted tree and on a tree rebuilt for it (SAH device build, one-frame launches at 1080p, Msamples/s, median of 5 x 24 frames) ==")
first, count = n // 2, n // 10
centre = centroid(tris0, first, count)
motions = {"a rotation of one part (10 % of the mesh) by 2 degrees": about(centre, rotation_y(np.radians(2.0))),
           "the same part carried across the scene": scene.part_move(0, 1, translation=(0.5 * ext, 0.1 * ext, 0.0))["m"].reshape(3, 4)}
ctx.build_scene(tris0, mats, method="sah")
r0 = statistics.median(frame_rate(ctx, cam))
print(f"rest pose, built tree                                        {r0:8.0f}")
for name, m in motions.items():
    moves = [(first, count, m)]
    ctx.build_scene(tris0, mats, method="sah")
    ctx.pose_parts(moves)
    a = statistics.median(frame_rate(ctx, cam))
    ctx.build_scene(scene.pose_parts(tris0, moves), mats, method="sah")
    b = statistics.median(frame_rate(ctx, cam))
    print(f"{name:56s} refitted {a:8.0f}   rebuilt {b:8.0f}   refitted / rebuilt = {a / b:.3f}")
ctx.close()
sys.exit(0 if ok else 1)
