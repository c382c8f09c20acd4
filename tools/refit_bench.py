#!/usr/bin/env python3
"""Run on the GPU box: what a pose change of the 1 M-triangle terrain costs (BVH context, 1920x1080) by the update form of rvpt_hip_upload_scene against the
only route there was before it — rvpt_bvh_build + a full upload_scene — and against the floor, a bare host-to-device copy of the same 48 MB; then what
traversal pays on a refitted tree against a freshly built one.  -> stdout (profiles/refit_update.txt)
usage: tools/refit_bench.py [all|updates|guard|guard-updates]     (updates: one upload and a few updates, nothing else — the run to put under rocprofv3
--kernel-trace --stats; guard: only the guarded update's section, -> profiles/guarded_update.txt; guard-updates: a device build and a few guarded updates, for the
same profiler run)
       tools/refit_bench.py --sparse 0.01 [updates]      the SPARSE update (Context.update_triangles(indices=)) of that fraction of the terrain beside the plain
update in the same run, from a host array and from device memory, one block contiguous in added order and the same number scattered -> profiles/sparse_update.txt;
exits non-zero unless the sparse update from a host array is quicker than the plain one.  With `updates`: a few sparse updates and nothing else, for the profiler"""
import statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rvpt_amd import Camera, RenderSettings, native, scene  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
sparse_fraction = float(sys.argv[2]) if what == "--sparse" and len(sys.argv) > 2 else 0.01
sparse_only_updates = what == "--sparse" and len(sys.argv) > 3 and sys.argv[3] == "updates"
W, H = 1920, 1080


def spread(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms   min {min(xs) * 1e3:9.3f}   max {max(xs) * 1e3:9.3f}   n {len(xs)}"


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def frame_rate(ctx, cam, frames=24, reps=5):
    """Msamples/s of one-frame launches (a moving mesh leaves nothing to batch), wall clock over `frames` frames, best-of and median of `reps`"""
    def run():
        for f in range(frames):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ctx.wait()
    ts = timed(run, reps)
    return [W * H * frames / t / 1e6 for t in ts]


def guard_section(tris0, mats, ext, cam):
    """The guarded update (Context.update_triangles(rebuild_above=)) on the 1 M-triangle terrain, built on the device, poses in a device tensor: what the guard adds
    to the plain update (same run, same context, interleaved), what a rebuild under it takes, and what the cost ratio says beside the traversal-rate ratio."""
    import math
    import torch
    print("\n== guarded update: plain | guarded, report only | guarded, rebuilding (wall clock of the call, device tensor, SAH device build; interleaved) ==")
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    ctx.build_scene(tris0, mats, method="sah")
    poses = [torch.from_numpy(scene.wobble(tris0, 0.5 + 0.9 * k, 0.02 * ext)).to("cuda:0") for k in range(2)]
    plain, guarded = [], []
    for it in range(23):
        for which, out in (("plain", plain), ("guarded", guarded)):
            t0 = time.perf_counter()
            ctx.update_triangles(poses[it % 2], rebuild_above=None if which == "plain" else math.inf)
            if it >= 3:
                out.append(time.perf_counter() - t0)
    print(f"plain update form                     {spread(plain)}")
    print(f"guarded, report only                  {spread(guarded)}")
    print(f"the guard adds (difference of medians) {(statistics.median(guarded) - statistics.median(plain)) * 1e6:8.1f} us")
    for method in ("lbvh", "ploc", "sah"):
        ctx.build_scene(tris0, mats, method=method)
        far = [torch.from_numpy(scene.wobble(tris0, 1.4 + 1.7 * k, 0.10 * ext)).to("cuda:0") for k in range(2)]
        rebuilds, n_rebuilt = [], 0
        for it in range(7):
            t0 = time.perf_counter()
            rep = ctx.update_triangles(far[it % 2], rebuild_above=1.0)  # every pose change of this size costs more than the tree built for the pose before it
            if it >= 1:
                rebuilds.append(time.perf_counter() - t0)
                n_rebuilt += int(rep.rebuilt)
        print(f"guarded, limit 1.0, {method:4s} ({n_rebuilt} of {len(rebuilds)} rebuilt)  {spread(rebuilds)}")
    print("\n== what the cost predicts: cost ratios beside the traversal-rate ratio (one-frame launches at 1080p, Msamples/s, median of 5 x 24 frames) ==")
    print("builder  amplitude   cost refit/base   cost fresh/base   cost refit/fresh   rate refit   rate fresh   rate refit/fresh")
    for method in ("lbvh", "ploc", "sah"):
        for amp in (0.02, 0.10):
            pose = scene.wobble(tris0, 1.4, amp * ext)
            dev = torch.from_numpy(pose).to("cuda:0")
            ctx.build_scene(tris0, mats, method=method)
            rep = ctx.update_triangles(dev, rebuild_above=math.inf)
            a = statistics.median(frame_rate(ctx, cam))
            ctx.build_scene(dev, mats, method=method)
            fresh = ctx.update_triangles(dev, rebuild_above=math.inf).base_cost
            b = statistics.median(frame_rate(ctx, cam))
            print(f"{method:7s}  {amp:9.2f}   {rep.ratio:15.4f}   {fresh / rep.base_cost:15.4f}   {rep.cost / fresh:16.4f}   {a:10.0f}   {b:10.0f}   {a / b:16.3f}")
    ctx.close()


def guard_updates(tris0, mats, ext):
    import math
    import torch
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    ctx.build_scene(tris0, mats, method="sah")
    poses = [torch.from_numpy(scene.wobble(tris0, 0.5 + 0.9 * k, 0.02 * ext)).to("cuda:0") for k in range(2)]
    for k in range(8):
        ctx.update_triangles(poses[k % 2], rebuild_above=math.inf)
    ctx.close()
    print("8 guarded updates done")


tris0, mats = scene.heightfield_scene()
ext = float(np.ptp(tris0.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
if what in ("guard", "guard-updates"):
    c = Camera(W / H)
    c.translation = np.array([0.0, 2.5, -5.0])
    c.rotation = np.array([0.0, 25.0, 0.0])
    print(f"scene: {tris0.shape[0]} triangles, extent {ext:.2f}")
    guard_section(tris0, mats, ext, c.get_data()) if what == "guard" else guard_updates(tris0, mats, ext)
    sys.exit(0)
t0 = time.perf_counter()
nodes, idx = native.build_bvh(tris0)
print(f"scene: {tris0.shape[0]} triangles, {nodes.shape[0]} nodes, extent {ext:.2f}; first rvpt_bvh_build {(time.perf_counter() - t0) * 1e3:.0f} ms (cold)")
tris = tris0[idx]
c = Camera(W / H)
c.translation = np.array([0.0, 2.5, -5.0])
c.rotation = np.array([0.0, 25.0, 0.0])
cam = c.get_data()
poses = [scene.wobble(tris, 0.5 + 0.9 * k, 0.02 * ext) for k in range(4)]  # in leaf order
ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
ctx.upload_scene(nodes, tris, mats)



def sparse_section(ctx, tris, idx, poses, fraction, only_updates):
    """The sparse update beside the plain one on ONE context (host-built tree: the lists are leaf-order positions).  `block`: k triangles contiguous in the order
    they were added, mapped through the inverse of the build's primitive indices; `scattered`: k positions drawn from the whole scene."""
    import torch
    n = tris.shape[0]
    k = max(1, int(round(fraction * n)))
    inverse = np.empty(n, dtype=np.int64)
    inverse[np.asarray(idx, dtype=np.int64)] = np.arange(n)
    rng = np.random.RandomState(9)
    start = int(rng.randint(0, n - k + 1))
    lists = {"block": inverse[start:start + k], "scattered": rng.permutation(n)[:k]}
    rows = {name: [np.ascontiguousarray(p[l]) for p in poses[:2]] for name, l in lists.items()}
    dev_rows = {name: [torch.from_numpy(r).to("cuda:0") for r in rs] for name, rs in rows.items()}
    dev_lists = {name: torch.from_numpy(l.astype(np.int32)).to("cuda:0") for name, l in lists.items()}
    it = [0]
    if only_updates:
        for name in lists:
            for _ in range(4):
                ctx.update_triangles(rows[name][it[0] % 2], indices=lists[name])
                ctx.update_triangles(dev_rows[name][it[0] % 2], indices=dev_lists[name]); it[0] += 1
        print(f"16 sparse updates of {k} triangles done")
        return True
    print(f"\n== sparse update of {k} of {n} triangles ({fraction:.4f}) beside the plain update, same context, same run (wall clock of the call, median of 20) ==")
    def plain_host():
        ctx.update_triangles(poses[it[0] % 4]); it[0] += 1
    dev_poses = [torch.from_numpy(p).to("cuda:0") for p in poses[:2]]
    def plain_dev():
        ctx.update_triangles(dev_poses[it[0] % 2]); it[0] += 1
    full_host, full_dev = timed(plain_host, 20, warm=3), timed(plain_dev, 20, warm=3)
    print(f"plain update, host numpy array          {spread(full_host)}")
    print(f"plain update, torch tensor on device    {spread(full_dev)}")
    ok = True
    for name in lists:
        def sparse_host():
            ctx.update_triangles(rows[name][it[0] % 2], indices=lists[name]); it[0] += 1
        def sparse_dev():
            ctx.update_triangles(dev_rows[name][it[0] % 2], indices=dev_lists[name]); it[0] += 1
        h, d = timed(sparse_host, 20, warm=3), timed(sparse_dev, 20, warm=3)
        span = int(lists[name].max() - lists[name].min() + 1)
        print(f"sparse, {name:9s} host arrays         {spread(h)}    (rows prepared: {span})")
        print(f"sparse, {name:9s} device memory       {spread(d)}")
        quicker = statistics.median(h) < statistics.median(full_host)
        print(f"        {name:9s} host: {statistics.median(full_host) / statistics.median(h):.1f} x the plain update from a host array -> {'ok' if quicker else 'NOT QUICKER'}")
        ok = ok and quicker
    return ok


if what == "--sparse":
    ok = sparse_section(ctx, tris, idx, poses, sparse_fraction, sparse_only_updates)
    ctx.close()
    sys.exit(0 if ok else 1)

if what == "updates":
    for k in range(8):
        ctx.update_triangles(poses[k % 4])
    ctx.close()
    print("8 updates done")
    sys.exit(0)

print("\n== cost of a pose change (wall clock, host call to return; the caller's array may be freed on return) ==")
k = [0]
def update():
    ctx.update_triangles(poses[k[0] % 4]); k[0] += 1
upd = timed(update, 20, warm=3)
print(f"update form (host numpy array)        {spread(upd)}")

import torch  # noqa: E402
dev_poses = [torch.from_numpy(p).to("cuda:0") for p in poses[:2]]
def update_dev():
    ctx.update_triangles(dev_poses[k[0] % 2]); k[0] += 1
upd_dev = timed(update_dev, 20, warm=3)
print(f"update form (torch tensor on device)  {spread(upd_dev)}    <- prepare_triangles + level sweep + wide gather + a device copy")

unsorted = [tris0.copy() for _ in range(2)]
for u, p in zip(unsorted, poses):
    u[idx] = p  # the pose in the order the triangles were added: what a caller without the update form starts from
def rebuild():
    u = unsorted[k[0] % 2]; k[0] += 1
    n2, i2 = native.build_bvh(u)
    ctx.upload_scene(n2, u[i2], mats)
def rebuild_parts():
    u = unsorted[k[0] % 2]; k[0] += 1
    a = time.perf_counter(); n2, i2 = native.build_bvh(u)
    b = time.perf_counter(); s = u[i2]
    c_ = time.perf_counter(); ctx.upload_scene(n2, s, mats)
    return b - a, c_ - b, time.perf_counter() - c_
base = timed(rebuild, 5, warm=1)
parts = [rebuild_parts() for _ in range(3)]
print(f"baseline: rvpt_bvh_build + upload     {spread(base)}")
print("          of which build / permute / upload_scene (ms): " + "; ".join(f"{a * 1e3:.0f} / {b * 1e3:.0f} / {c_ * 1e3:.0f}" for a, b, c_ in parts))
def refit_route():
    p = poses[k[0] % 4]; k[0] += 1
    ctx.upload_scene(scene.refit_bvh(nodes, p), p, mats)
print(f"numpy refit_bvh + full upload         {spread(timed(refit_route, 3, warm=0))}")

dst48 = torch.empty(tris.shape[0] * 48, dtype=torch.uint8, device="cuda:0")
dst64 = torch.empty(tris.shape[0] * 64, dtype=torch.uint8, device="cuda:0")
src48 = torch.from_numpy(np.frombuffer(np.random.RandomState(1).bytes(tris.shape[0] * 48), dtype=np.uint8).copy())  # pageable, like a numpy array
src64 = torch.from_numpy(poses[0].view(np.uint8).reshape(-1))
def copy48():
    dst48.copy_(src48); torch.cuda.synchronize()
def copy64():
    dst64.copy_(src64); torch.cuda.synchronize()
fl48, fl64 = timed(copy48, 20, warm=3), timed(copy64, 20, warm=3)
print(f"floor: flat H2D copy of 48 MB         {spread(fl48)}    (pageable host memory, {tris.shape[0] * 48 / 1e6 / statistics.median(fl48) / 1e3:.1f} GB/s)")
print(f"       flat H2D copy of 64 MB         {spread(fl64)}")
m_u, m_d, m_b, m_f = (statistics.median(x) for x in (upd, upd_dev, base, fl48))
print(f"summary: update {m_u * 1e3:.2f} ms = {m_b / m_u:.0f} x faster than rebuild + upload ({m_b * 1e3:.0f} ms), {m_u / m_f:.2f} x the 48 MB copy floor ({m_f * 1e3:.2f} ms); "
      f"the device-side part (device source) {m_d * 1e3:.2f} ms, so the strided host copy holds about {(m_u - m_d) * 1e3:.2f} ms")

print("\n== what refitting costs in traversal: the same deformed geometry on the refitted tree and on a freshly built one (one-frame launches, Msamples/s) ==")
ctx.upload_scene(nodes, tris, mats)
r0 = frame_rate(ctx, cam)
print(f"undeformed, built tree                     median {statistics.median(r0):8.0f}   min {min(r0):8.0f}   max {max(r0):8.0f}")
for amp in (0.02, 0.1):
    pose = scene.wobble(tris, 1.4, amp * ext)
    ctx.upload_scene(nodes, tris, mats)
    ctx.update_triangles(pose)
    a = frame_rate(ctx, cam)
    u = tris0.copy(); u[idx] = pose
    n2, i2 = native.build_bvh(u)
    ctx.upload_scene(n2, u[i2], mats)
    b = frame_rate(ctx, cam)
    print(f"amplitude {amp:4.2f} x extent: refitted tree    median {statistics.median(a):8.0f}   min {min(a):8.0f}   max {max(a):8.0f}")
    print(f"                         rebuilt tree     median {statistics.median(b):8.0f}   min {min(b):8.0f}   max {max(b):8.0f}    refit / rebuilt = {statistics.median(a) / statistics.median(b):.3f}")
ctx.close()
guard_section(tris0, mats, ext, cam)
