#!/usr/bin/env python3
"""Run on the GPU box: what a REBUILD of the 1 M-triangle terrain's tree costs (BVH context, 1920x1080) by the build form of rvpt_hip_upload_scene against the
only route there was before it — rvpt_bvh_build + permute + a full upload_scene — and against the floor, a bare host-to-device copy of the same 64 MB; then
what traversal pays on the device-built LBVH against the binned-SAH tree of rvpt_bvh_build and against a refitted tree.  -> stdout (profiles/device_build.txt)
usage: tools/build_bench.py [--method lbvh|ploc|sah] [all|builds|traversal|stages <kernel_stats.csv> [n_builds]]
    --method sah: rvpt_bvh_build's binned-SAH tree made on the device (profiles/device_build_sah.txt).  all: its build time beside the LBVH's and
        the host route's in the same run (asserted: from a device tensor below the host route's); traversal: four trees interleaved — SAH-device, PLOC, LBVH,
        rvpt_bvh_build's — one context each
    --method ploc: the PLOC tree of the build form (profiles/device_build_ploc.txt).  all: its build time beside the LBVH's in the same run;
        builds: PLOC builds; traversal: three trees interleaved on one box — PLOC, LBVH, rvpt_bvh_build's — one context each, a repetition of each in turn
    builds: one upload and a few device builds from a device tensor, nothing else — the run to put under rocprofv3 --kernel-trace --stats
    traversal: the traversal table only (what the leaf-size sweep runs per library)
    stages: no GPU — the per-stage table of profiles/device_build.txt from the kernel_stats.csv of such a rocprofv3 run
how profiles/device_build.txt is made (one box, one run; the parts are concatenated in this order):
    python -m rvpt_amd.build --leaf-variant 4; python -m rvpt_amd.build --leaf-variant 8        (where hipcc is: rvpt_amd/librvpt_hip_leaf<L>.so)
    tools/build_bench.py all
    RVPT_HIP_LIB=rvpt_amd/librvpt_hip_leaf4.so LEAF_TRIS=4 tools/build_bench.py traversal      (and the same with 8)
    rocprofv3 --kernel-trace --stats -d <dir> -o builds --output-format csv -- python tools/build_bench.py builds
    tools/build_bench.py stages <dir>/builds_kernel_stats.csv"""
import os, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

METHOD = "lbvh"
if "--method" in sys.argv:
    at = sys.argv.index("--method")
    METHOD = sys.argv[at + 1]
    del sys.argv[at:at + 2]
    if METHOD not in ("lbvh", "ploc", "sah"):
        sys.exit("--method lbvh|ploc|sah")

STAGES = {"sah_init": "SAH boxes, centroids, iota", "sah_large": "SAH node + bin reduction (large nodes)", "sah_decide": "SAH node + bin reduction (one wave per node) and decision",
          "sah_emit": "SAH emit", "sah_flags": "SAH partition", "sah_scatter": "SAH partition", "sah_median": "SAH median sort", "gather_records_by_index": "gather",
          "ploc_init": "PLOC clusters", "ploc_nearest": "PLOC nearest neighbour", "ploc_keep": "PLOC merge + compaction", "ploc_merge": "PLOC merge + compaction", "ploc_tail": "PLOC tail (one work-group)",
          "layout_root": "topology", "layout_level": "topology", "validate_materials": "validate", "reset_counters": "keys", "centroid_bounds": "keys", "make_keys": "keys", "gather_records": "gather", "root_level": "topology",
          "emit_level": "topology", "refit_level": "boxes", "wide_root": "wide form", "wide_pick": "wide form", "wide_emit": "wide form", "wide_heads": "wide form",
          "wide_need": "wide form", "refit_wide_gather": "wide form", "prepare_triangles": "prepare", "prepare_materials": "prepare",
          "copyBuffer": "copies (read-backs of one word, materials)", "fillBuffer": "memset"}


def stages(csv_path, n_builds=8):
    """the kernels and copies of a `builds` run under rocprofv3 --kernel-trace --stats, grouped by stage of the build, per build"""
    import csv
    rows = list(csv.DictReader(open(csv_path)))
    agg = {}
    for r in rows:
        key = next((v for k, v in STAGES.items() if k in r["Name"]), None)
        if key is None:
            key = "rocPRIM (radix sort of the keys + the scans of the level loops)" if "rocprim" in r["Name"] else "other (torch's copies of the source tensors)"
        a = agg.setdefault(key, [0, 0.0])
        a[0] += int(r["Calls"]); a[1] += float(r["TotalDurationNs"])
    print(f"# ---- the device part by stage: rocprofv3 --kernel-trace --stats of `tools/build_bench.py builds` ({n_builds} device builds of the 1 M-triangle terrain from a "
          f"device tensor), per build ----")
    for k, (calls, ns) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print(f"{k:75s} {calls / n_builds:7.1f} launches  {ns / n_builds / 1e3:9.1f} us")
    print(f"{'sum of kernel and copy durations':75s} {'':16s}  {sum(a[1] for a in agg.values()) / n_builds / 1e3:9.1f} us")
    print("# top kernels (name, calls over all builds, average us):")
    for r in rows[:12]:
        print(f"#   {r['Name'][:100]:100s} {r['Calls']:>5s} {float(r['AverageNs']) / 1e3:8.1f}")


if len(sys.argv) > 2 and sys.argv[1] == "stages":
    stages(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 8)
    sys.exit(0)

from rvpt_amd import Camera, RenderSettings, native, scene  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "all"
W, H = 1920, 1080


def spread(xs):
    return f"median {statistics.median(xs) * 1e3:9.3f} ms   min {min(xs) * 1e3:9.3f}   max {max(xs) * 1e3:9.3f}   n {len(xs)}"


def rates(xs):
    return f"median {statistics.median(xs):8.0f}   min {min(xs):8.0f}   max {max(xs):8.0f}"


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def frame_rate(ctx, cam, w, h, frames=24, reps=5):
    """Msamples/s of one-frame launches (a moving mesh leaves nothing to batch), wall clock over `frames` frames"""
    def run():
        for f in range(frames):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ctx.wait()
    return [w * h * frames / t / 1e6 for t in timed(run, reps)]


def terrain_camera(w, h):
    c = Camera(w / h)
    c.translation = np.array([0.0, 2.5, -5.0])
    c.rotation = np.array([0.0, 25.0, 0.0])
    return c.get_data()


print(f"library: {native.lib_path().name}")
tris0, mats = scene.heightfield_scene()
ext = float(np.ptp(tris0.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
cam = terrain_camera(W, H)
ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
poses = [scene.wobble(tris0, 0.5 + 0.9 * k, 0.02 * ext) for k in range(2)]  # in the order the triangles were made

if what == "builds":
    import torch
    dev = [torch.from_numpy(p).to("cuda:0") for p in poses]
    for k in range(8):
        ctx.build_scene(dev[k % 2], mats, method=METHOD)
    ctx.close()
    print(f"8 device builds ({METHOD}) done")
    sys.exit(0)

if what == "all":
    import torch
    print(f"scene: {tris0.shape[0]} triangles, extent {ext:.2f}")
    import ctypes
    temp = ctypes.c_size_t(0)  # rv::build_temp_bytes (rvpt_build.h) by its mangled name: what the library allocates as d_build_temp for this many triangles
    fn = native.load()._ZN2rv16build_temp_bytesEjPm
    fn.argtypes, fn.restype = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int
    assert fn(tris0.shape[0], ctypes.byref(temp)) == 0
    n_ = tris0.shape[0]
    print(f"device build buffers: keys + ranges + flags (d_build) {(24 * n_ + 3 * (((n_ + 1) * 4 + 15) & ~15)) / 1e6:.2f} MB, permutation (d_perm) {4 * n_ / 1e6:.2f} MB, "
          f"sort scratch (d_build_temp, rocPRIM's answer) {temp.value / 1e6:.3f} MB = {temp.value} bytes, node buffer worst case {(2 * n_ + 2) * 32 / 1e6:.2f} MB")
    print("\n== cost of a rebuild (wall clock, host call to return; the caller's array may be freed on return) ==")
    k = [0]
    def host_route():
        u = poses[k[0] % 2]; k[0] += 1
        n2, i2 = native.build_bvh(u)
        ctx.upload_scene(n2, u[i2], mats)
    def host_route_parts():
        u = poses[k[0] % 2]; k[0] += 1
        a = time.perf_counter(); n2, i2 = native.build_bvh(u)
        b = time.perf_counter(); s = u[i2]
        c_ = time.perf_counter(); ctx.upload_scene(n2, s, mats)
        return b - a, c_ - b, time.perf_counter() - c_
    def build_host():
        ctx.build_scene(poses[k[0] % 2], mats); k[0] += 1
    dev = [torch.from_numpy(p).to("cuda:0") for p in poses]
    def build_dev():
        ctx.build_scene(dev[k[0] % 2], mats); k[0] += 1
    base = timed(host_route, 5, warm=1)
    parts = [host_route_parts() for _ in range(3)]
    print(f"rvpt_bvh_build + permute + upload      {spread(base)}")
    print("          of which build / permute / upload_scene (ms): " + "; ".join(f"{a * 1e3:.0f} / {b * 1e3:.0f} / {c_ * 1e3:.0f}" for a, b, c_ in parts))
    bh = timed(build_host, 20, warm=3)
    print(f"build form (host numpy array)          {spread(bh)}")
    bd = timed(build_dev, 20, warm=3)
    print(f"build form (torch tensor on device)    {spread(bd)}    <- keys, sort, gather, level loops, boxes, wide form, prepare_triangles")
    dst64 = torch.empty(tris0.shape[0] * 64, dtype=torch.uint8, device="cuda:0")
    src64 = torch.from_numpy(poses[0].view(np.uint8).reshape(-1))
    def copy64():
        dst64.copy_(src64); torch.cuda.synchronize()
    fl = timed(copy64, 20, warm=3)
    print(f"floor: flat H2D copy of 64 MB          {spread(fl)}    (pageable host memory, {tris0.shape[0] * 64 / 1e6 / statistics.median(fl) / 1e3:.1f} GB/s)")
    if METHOD == "ploc":
        def ploc_host():
            ctx.build_scene(poses[k[0] % 2], mats, method="ploc"); k[0] += 1
        def ploc_dev():
            ctx.build_scene(dev[k[0] % 2], mats, method="ploc"); k[0] += 1
        ph = timed(ploc_host, 20, warm=3)
        print(f"PLOC build form (host numpy array)     {spread(ph)}")
        pd = timed(ploc_dev, 20, warm=3)
        print(f"PLOC build form (torch tensor)         {spread(pd)}")
        print(f"PLOC / LBVH build time: host array {statistics.median(ph) / statistics.median(bh):.2f}, device tensor {statistics.median(pd) / statistics.median(bd):.2f}")
    if METHOD == "sah":
        def sah_host():
            ctx.build_scene(poses[k[0] % 2], mats, method="sah"); k[0] += 1
        def sah_dev():
            ctx.build_scene(dev[k[0] % 2], mats, method="sah"); k[0] += 1
        sh = timed(sah_host, 20, warm=3)
        print(f"SAH build form (host numpy array)      {spread(sh)}")
        sd = timed(sah_dev, 20, warm=3)
        print(f"SAH build form (torch tensor)          {spread(sd)}")
        print(f"SAH / LBVH build time: host array {statistics.median(sh) / statistics.median(bh):.2f}, device tensor {statistics.median(sd) / statistics.median(bd):.2f}; "
              f"host route / SAH from a device tensor {statistics.median(base) / statistics.median(sd):.1f}")
        assert statistics.median(sd) < statistics.median(base), "the SAH build form from a device pointer must take less wall time than the host route"
    m_b, m_h, m_d, m_f = (statistics.median(x) for x in (base, bh, bd, fl))
    print(f"summary: build form from a host array {m_h * 1e3:.2f} ms = {m_b / m_h:.1f} x faster than rvpt_bvh_build + upload ({m_b * 1e3:.0f} ms), {m_h / m_f:.2f} x the 64 MB copy floor "
          f"({m_f * 1e3:.2f} ms); from a device tensor {m_d * 1e3:.2f} ms")
    assert m_h < m_b, "the build form from a host array must take less wall time than the host route"
    del dev, dst64

if METHOD == "sah":
    print("\n== traversal: rvpt_bvh_build's tree made on the device (SAH-device) against the PLOC tree, the LBVH and the host-built tree (one-frame launches, Msamples/s) ==")
elif METHOD == "ploc":
    print(f"\n== traversal: the PLOC tree (radius {scene.PLOC_RADIUS}, leaves of 1) against the LBVH (leaves of <= {scene.LBVH_LEAF_TRIS}) and rvpt_bvh_build's binned-SAH tree (one-frame launches, Msamples/s) ==")
else:
    print(f"\n== traversal: the device-built LBVH (leaves of <= {os.environ.get('LEAF_TRIS', scene.LBVH_LEAF_TRIS)}) against rvpt_bvh_build's binned-SAH tree (one-frame launches, Msamples/s) ==")
def compare_three(name, tris, ms, c, w, h, amps=()):
    """PLOC, LBVH and the host's binned-SAH tree of one pose, a context each; five rounds, every round one repetition of each tree in turn"""
    e = float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
    for amp in (0.0,) + tuple(amps):
        pose = scene.wobble(tris, 1.4, amp * e) if amp else tris
        cxs = {k_: native.Context(w, h, 0, 0, 1, native.TRAVERSAL_BVH) for k_ in (("sah",) if METHOD == "sah" else ()) + ("ploc", "lbvh", "host")}
        if METHOD == "sah":
            t0 = time.perf_counter(); cxs["sah"].build_scene(pose, ms, method="sah"); t_sah = time.perf_counter() - t0
        t0 = time.perf_counter(); tree = cxs["ploc"].build_scene(pose, ms, method="ploc"); t_ploc = time.perf_counter() - t0
        t0 = time.perf_counter(); cxs["lbvh"].build_scene(pose, ms); t_lbvh = time.perf_counter() - t0
        t0 = time.perf_counter(); n2, i2 = native.build_bvh(pose); cxs["host"].upload_scene(n2, pose[i2], ms); t_host = time.perf_counter() - t0
        got = {k_: [] for k_ in cxs}
        for _ in range(5):
            for k_, cx in cxs.items():
                got[k_] += frame_rate(cx, c, w, h, reps=1)
        for cx in cxs.values():
            cx.close()
        med = {k_: statistics.median(v) for k_, v in got.items()}
        pad = f"{'':{len(name) + 18}}"
        line = (f"{name}, amplitude {amp:4.2f}: PLOC ({tree})  {rates(got['ploc'])}\n{pad}LBVH         {rates(got['lbvh'])}\n{pad}host-built   {rates(got['host'])}\n"
                f"{pad}PLOC / LBVH = {med['ploc'] / med['lbvh']:.3f}   PLOC / host = {med['ploc'] / med['host']:.3f}   LBVH / host = {med['lbvh'] / med['host']:.3f}")
        if METHOD == "sah":
            line = (f"{name}, amplitude {amp:4.2f}: SAH-device   {rates(got['sah'])}\n{pad}" + line.split(": ", 1)[1] +
                    f"\n{pad}SAH-device / host = {med['sah'] / med['host']:.3f}   (five rounds; host-built spread {min(got['host']) / med['host']:.3f} .. {max(got['host']) / med['host']:.3f} of its median)"
                    f"\n{pad}rebuild {t_sah * 1e3:.1f} ms (SAH-device, first call of a context) vs {t_host * 1e3:.1f} ms (host)")
        for label, t_dev, r in (("PLOC", t_ploc, med["ploc"]), ("LBVH", t_lbvh, med["lbvh"])):
            per_dev, per_host = w * h / r / 1e6, w * h / med["host"] / 1e6
            line += f"\n{pad}rebuild {t_dev * 1e3:.1f} ms ({label}, first call of a context) vs {t_host * 1e3:.1f} ms (host): "
            line += f"the host rebuild overtakes after {(t_host - t_dev) / (per_dev - per_host):.0f} one-frame launches" if per_dev > per_host and t_host > t_dev else "the host rebuild never overtakes" if t_host > t_dev else "the host route is no slower to build at this size"
        print(line, flush=True)


def compare(name, tris, ms, c, w, h, amps=()):
    if METHOD in ("ploc", "sah"):
        return compare_three(name, tris, ms, c, w, h, amps)
    cx = native.Context(w, h, 0, 0, 1, native.TRAVERSAL_BVH)
    e = float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())
    nodes, idx = native.build_bvh(tris)
    for amp in (0.0,) + tuple(amps):
        pose = scene.wobble(tris, 1.4, amp * e) if amp else tris
        t0 = time.perf_counter(); cx.build_scene(pose, ms); t_dev = time.perf_counter() - t0
        dev = frame_rate(cx, c, w, h)
        t0 = time.perf_counter(); n2, i2 = native.build_bvh(pose); cx.upload_scene(n2, pose[i2], ms); t_host = time.perf_counter() - t0
        host = frame_rate(cx, c, w, h)
        line = f"{name}, amplitude {amp:4.2f}: device-built {rates(dev)}\n{'':{len(name) + 18}}host-built   {rates(host)}    device / host = {statistics.median(dev) / statistics.median(host):.3f}"
        if amp:
            cx.upload_scene(nodes, tris[idx], ms)
            cx.update_triangles(pose[idx])
            ref = frame_rate(cx, c, w, h)
            line += f"\n{'':{len(name) + 18}}refitted     {rates(ref)}    refit / host = {statistics.median(ref) / statistics.median(host):.3f}"
        # frames after which the host rebuild has caught up: t_host + f / r_host = t_dev + f / r_dev
        per_dev, per_host = w * h / statistics.median(dev) / 1e6, w * h / statistics.median(host) / 1e6
        if per_dev > per_host:
            line += f"\n{'':{len(name) + 18}}rebuild {t_dev * 1e3:.1f} ms (device) vs {t_host * 1e3:.1f} ms (host): the host rebuild overtakes after {(t_host - t_dev) / (per_dev - per_host):.0f} one-frame launches"
        else:
            line += f"\n{'':{len(name) + 18}}rebuild {t_dev * 1e3:.1f} ms (device) vs {t_host * 1e3:.1f} ms (host): the host rebuild never overtakes"
        if t_host <= t_dev:
            line = line.rsplit("\n", 1)[0] + f"\n{'':{len(name) + 18}}rebuild {t_dev * 1e3:.1f} ms (device) vs {t_host * 1e3:.1f} ms (host): the host route is no slower to build at this size"
        print(line, flush=True)
    cx.close()

ctx.close()
compare("terrain 1 M 1080p", tris0, mats, cam, W, H, amps=(0.02, 0.1))
ct, cm = scene.cornell_scene()
c = Camera(W / H)
c.translation = np.array([0.0, 2.0, -1.9])
compare("Cornell + 9 k 1080p", ct, cm, c.get_data(), W, H)
dt, dm = scene.default_scene()
ident = np.zeros(20, np.float32)
ident[[0, 5, 10, 15]] = 1.0
ident[16], ident[17], ident[18] = W / H, np.pi / 2, 4.0
compare("default scene 1080p", dt, dm, ident, W, H)
