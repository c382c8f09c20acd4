#!/usr/bin/env python3
"""Run on the GPU box: what the SKIN UPDATE of rvpt_hip_upload_scene (Context.bind_skin, Context.skin) costs on the 1 M-triangle terrain (BVH context,
1920x1080, after build_scene(method="sah")), beside the yardsticks of the same run — the plain update form from a host array and from a device tensor, and a
whole-mesh pose update.  Candidates: the skin update from host bones and from device bones at 16, 64 and 1024 bones.  All alternate inside one loop (wall clock
of the call, median of 20 after 3 warm-up rounds; the binding of a candidate's bone count is made outside the timed call).  Then the bind itself, from host and
from device memory, and the kernel resources from the compiler's metadata.  -> stdout (profiles/skin_update.txt)
Nothing here is a pass/fail bar: the two expectations of the header are printed beside the numbers.
usage: tools/skin_bench.py [all|skin|guard]     (skin: the skin updates alone, for a second library named by RVPT_HIP_LIB — the global-load form of the kernel,
profiles/skin_update_exp_global_bones.patch — whose lines go beside the first run's; guard: the GUARDED SKIN UPDATE (Context.skin(rebuild_above=)) alone ->
stdout (profiles/guarded_skin.txt): what the guard adds to a plain skin, both alternating in one loop on one context; what a guarded skin that rebuilds costs,
per builder; and the ratio a bend of the bone grid reports.  Expected before the run: the guard adds about what it adds to a pose, 0.045 ms
(profiles/guarded_pose.txt: the same two cost kernels and one 8-byte read), and a rebuild costs about the guarded pose's, 2.2 / 3.5 / 15.1 ms)"""
import math, os, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rvpt_amd import native, scene  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
W, H = 1920, 1080
BONES = (16, 64, 1024)


def spread(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms   min {min(xs) * 1e3:9.3f}   max {max(xs) * 1e3:9.3f}   n {len(xs)}"


def rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def about(centre, rot):
    c = np.asarray(centre, dtype=np.float64)
    return np.concatenate([rot, (c - rot @ c).reshape(3, 1)], axis=1)


def weights(tris, k):
    """k bones on a sqrt(k) x sqrt(k) grid over x and z (a bending terrain patch): every vertex takes the four corners of its cell with bilinear weights, so a
    wave's 64 vertices touch a handful of bones and all four influences count"""
    p = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)
    g = int(round(np.sqrt(k)))
    assert g * g == k and g >= 2
    lo, hi = p.min(axis=0), p.max(axis=0)
    u = (p[:, 0] - lo[0]) / (hi[0] - lo[0]) * (g - 1)
    v = (p[:, 2] - lo[2]) / (hi[2] - lo[2]) * (g - 1)
    iu, iv = np.minimum(u.astype(np.int64), g - 2), np.minimum(v.astype(np.int64), g - 2)
    fu, fv = u - iu, v - iv
    rec = np.zeros(p.shape[0], dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"] = np.stack([iv * g + iu, iv * g + iu + 1, (iv + 1) * g + iu, (iv + 1) * g + iu + 1], axis=1)
    rec["weight"] = np.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], axis=1).astype(np.float32)
    return rec


def bones(tris, k, flip):
    p = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)
    g = int(round(np.sqrt(k)))
    lo, hi = p.min(axis=0), p.max(axis=0)
    out = np.zeros((k, 3, 4), dtype=np.float32)
    for b in range(k):
        c = np.array([lo[0] + (b % g) / (g - 1) * (hi[0] - lo[0]), 0.5 * (lo[1] + hi[1]), lo[2] + (b // g) / (g - 1) * (hi[2] - lo[2])])
        m = about(c, rotation_y((0.02 if flip else -0.02) * (1 + b % 3)))
        m[1, 3] += 0.01 * np.sin(0.7 * b + flip)
        out[b] = m
    return out


tris0, mats = scene.heightfield_scene()
n = tris0.shape[0]
ext = float(np.ptp(tris0.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
print(f"scene: {n} triangles, extent {ext:.2f}; library: {os.environ.get('RVPT_HIP_LIB') or 'rvpt_amd/librvpt_hip.so'}")
import torch  # noqa: E402

ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
ctx.build_scene(tris0, mats, method="sah")


def bend(tris, k, amplitude, sign):
    """the bones of `bones` with the middle column of the grid carried along z by `sign` x `amplitude`, its neighbours by half of that: the patch folds along a line"""
    g = int(round(np.sqrt(k)))
    out = bones(tris, k, 0)
    for b in range(k):
        d = abs(b % g - g // 2)
        if d <= 1:
            out[b, 2, 3] += np.float32(sign * amplitude * (1.0 if d == 0 else 0.5))
    return out


def guard_section():
    k = 64
    rec = weights(tris0, k)
    d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1, 32).copy()).to("cuda:0")
    ctx.bind_skin(d_rec)
    gentle = [bones(tris0, k, f) for f in (0, 1)]
    variants = {"plain skin, 64 bones, host array": lambda j: ctx.skin(gentle[j]),
                "guarded skin, report only, the same bones": lambda j: ctx.skin(gentle[j], rebuild_above=math.inf),
                "guarded skin, limit 1.1 (never reached), the same bones": lambda j: ctx.skin(gentle[j], rebuild_above=1.1)}
    times = {name: [] for name in variants}
    ratios = []
    for it in range(23):  # the candidate and its yardstick alternate: whatever drifts, drifts for both
        for name, fn in variants.items():
            t0 = time.perf_counter()
            rep = fn(it % 2)
            if it >= 3:
                times[name].append(time.perf_counter() - t0)
            assert rep is None or not rep.rebuilt
            if rep is not None:
                ratios.append(rep.ratio)
    print(f"\n== the guard's cost: {n} triangles, {k} bones on a grid with bilinear weights, SAH device build (wall clock of the call; alternating in one loop on one context) ==")
    for name, ts in times.items():
        print(f"{name:56s} {spread(ts)}")
    med = {name: statistics.median(ts) for name, ts in times.items()}
    plain = med["plain skin, 64 bones, host array"]
    print(f"guarded (report only) - plain = {(med['guarded skin, report only, the same bones'] - plain) * 1e3:.3f} ms (expected: about the 0.045 ms of the guarded pose);   "
          f"guarded / plain = {med['guarded skin, report only, the same bones'] / plain:.2f};   ratios reported by the gentle bones: {min(ratios):.4f} .. {max(ratios):.4f}")

    print("\n== a guarded skin that rebuilds (limit 1.0; the middle column of the bone grid carried half the extent along z and against it in turn, each on the tree "
          "built for the other; wall clock of the call; expected: about the guarded pose's 2.2 / 3.5 / 15.1 ms) ==")
    folds = [bend(tris0, k, 0.5 * ext, s) for s in (1.0, -1.0)]
    for method in ("lbvh", "ploc", "sah"):
        built = ctx.build_scene(tris0, mats, method=method)
        ctx.bind_skin(d_rec)
        ts, kept = [], 0
        for it in range(7):
            t0 = time.perf_counter()
            rep = ctx.skin(folds[it % 2], rebuild_above=1.0)
            dt = time.perf_counter() - t0
            if rep.rebuilt and it >= 1:
                ts.append(dt)
            kept += not rep.rebuilt
        print(f"{method:5s} (the scene holds: {built:4s}) " + (spread(ts) if ts else "never rebuilt") + f"   calls that refitted: {kept} of 7")

    print("\n== the ratio a bend of the bone grid reports (SAH device build of the rest pose, report only; the middle column of the 8 x 8 grid carried along z by the "
          "given share of the extent, its two neighbours by half of that, over the gentle bones) ==")
    for share in (0.01, 0.05, 0.1, 0.25, 0.5):
        ctx.build_scene(tris0, mats, method="sah")
        ctx.bind_skin(d_rec)
        rep = ctx.skin(bend(tris0, k, share * ext, 1.0), rebuild_above=math.inf)
        print(f"bend of {share:5.2f} x extent   cost {rep.cost:12.4f}   base {rep.base_cost:12.4f}   ratio {rep.ratio:8.4f}")


if what == "guard":
    guard_section()
    ctx.close()
    sys.exit(0)

recs = {k: weights(tris0, k) for k in BONES}
mats_h = {k: [bones(tris0, k, f) for f in (0, 1)] for k in BONES}
mats_d = {k: [torch.from_numpy(m).to("cuda:0") for m in mats_h[k]] for k in BONES}

variants = {}
if what == "all":
    poses = [scene.wobble(tris0, 0.5 + 0.9 * j, 0.02 * ext) for j in range(2)]
    dev_poses = [torch.from_numpy(p).to("cuda:0") for p in poses]
    c0 = tris0.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64).mean(axis=0)
    whole = [scene.part_moves([(0, n, about(c0, rotation_y(a)))]) for a in (-0.02, 0.02)]
    variants["plain update, host numpy array"] = lambda j: ctx.update_triangles(poses[j])
    variants["plain update, torch tensor on device"] = lambda j: ctx.update_triangles(dev_poses[j])
    variants["pose, 1 part of everything"] = lambda j: ctx.pose_parts(whole[j])
for k in BONES:
    variants[f"skin, {k:4d} bones, host array"] = (lambda kk: lambda j: ctx.skin(mats_h[kk][j]))(k)
    variants[f"skin, {k:4d} bones, torch tensor on device"] = (lambda kk: lambda j: ctx.skin(mats_d[kk][j]))(k)
d_recs = {k: torch.from_numpy(recs[k].view(np.uint8).reshape(-1, 32).copy()).to("cuda:0") for k in BONES}
times = {name: [] for name in variants}
bound = None
for it in range(23):  # the candidates and the yardsticks alternate: whatever drifts, drifts for all of them
    for name, fn in variants.items():
        if name.startswith("skin"):
            k = int(name.split()[1])
            if bound != k:  # (outside the timed call: a device-to-device copy of 96 MB)
                ctx.bind_skin(d_recs[k])
                bound = k
        t0 = time.perf_counter()
        fn(it % 2)
        if it >= 3:
            times[name].append(time.perf_counter() - t0)
print(f"\n== after build_scene(method='sah'): {n} triangles (wall clock of the call, host call to return; alternating in one loop) ==")
for name, ts in times.items():
    print(f"{name:44s} {spread(ts)}")
med = {name: statistics.median(ts) for name, ts in times.items()}
if what == "all":
    host, dev, pose = med["plain update, host numpy array"], med["plain update, torch tensor on device"], med["pose, 1 part of everything"]
    for k in BONES:
        s = med[f"skin, {k:4d} bones, host array"]
        print(f"skin from host bones, {k:4d}: / plain update from a host array = {s / host:.3f};   / plain update from device memory = {s / dev:.2f} "
              f"({'nearer the device form' if abs(s - dev) < abs(s - host) else 'NEARER THE HOST FORM'});   / whole-mesh pose = {s / pose:.2f} (the price of blending)")

    print("\n== the bind (wall clock of the call; 96 bytes per triangle; the check of the bone indices included: a host loop, or one kernel and one read of four words) ==")
    for label, src in (("bind, host array", recs[64]), ("bind, torch tensor on device", d_recs[64])):
        ts = []
        for it in range(8):
            t0 = time.perf_counter()
            ctx.bind_skin(src)
            if it >= 2:
                ts.append(time.perf_counter() - t0)
        print(f"{label:44s} {spread(ts)}")

    sys.path.insert(0, str(ROOT / "tools"))
    from kernel_resources import kernel_resources  # noqa: E402
    print("\n== kernel resources (the compiler's own metadata, gfx950: rvpt_refit.hip) ==")
    print(f"  {'kernel':88s}  vgpr  sgpr  scratch static_lds")
    for name, r in sorted(kernel_resources(("rvpt_refit.hip",)).items()):
        if name.startswith(("skin_", "pose_parts", "rest_to")):
            print(f"  {name[:88]:88s} {r['vgpr']:5d} {r['sgpr']:5d} {r['scratch_bytes']:8d} {r['static_lds_bytes']:10d}")
ctx.close()
