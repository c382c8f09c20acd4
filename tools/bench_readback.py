#!/usr/bin/env python3
"""The geometry read-back (rvpt_hip_read with FORMAT_TRIANGLES and FORMAT_SURFACE_POINTS) measured -> profiles/scene_readback.txt.

usage: tools/bench_readback.py rates                    on the GPU box, on the 1 M-triangle terrain after build_scene("sah") (a context with a permutation):
                                                        the triangle read into device memory beside a flat device-to-device copy of the same bytes, into a
                                                        host array beside a flat device-to-host copy into pageable memory, and 2^20 surface records from device
                                                        and from host memory, prim in random order and in stored order — median of 7, wall clock of the call
       tools/bench_readback.py resources <parent tree>  where hipcc and a checkout of the parent commit are: VGPR, SGPR, scratch and static LDS of every
                                                        kernel of every .hip file there and here (tools/kernel_resources.py), and of the new kernel
Each mode rewrites its own section of profiles/scene_readback.txt and leaves the other."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "profiles" / "scene_readback.txt"
MARK = "==== kernel resources"
N = 1 << 20


def write_section(text, resources):
    old = OUT.read_text() if OUT.exists() else ""
    head, _, tail = old.partition(MARK)
    if resources:
        OUT.write_text(head.rstrip("\n") + ("\n\n" if head.strip() else "") + MARK + text)
    else:
        OUT.write_text(text.rstrip("\n") + "\n" + ("\n" + MARK + tail if tail else ""))


def timed(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def row(label, ts, nbytes=None, n=None):
    med = statistics.median(ts)
    what = f"{nbytes / med / 1e9:8.1f} GB/s" if nbytes is not None else f"{n / med / 1e6:8.1f} Mrecords/s"
    return f"{label:64s} median {med * 1e3:9.3f} ms   min {min(ts) * 1e3:9.3f}   max {max(ts) * 1e3:9.3f}   {what}"


def rates():
    import torch
    from rvpt_amd import native, scene
    tris, mats = scene.heightfield_scene()
    tris = np.ascontiguousarray(tris)
    n = tris.shape[0]
    nbytes = n * 64
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    assert ctx.build_scene(tris, mats, "sah") == "sah"
    lines = ["geometry read-back: tools/bench_readback.py rates",
             f"the terrain: {n} triangles ({nbytes / 1e6:.1f} MB of rows), build_scene(sah): the stored order is the builder's, every read goes through the permutation",
             "one MI355X; median of 7 after 2 warm calls, wall clock around the call (it returns after its stream has finished)", "",
             "== RVPT_HIP_FORMAT_TRIANGLES =="]
    dev = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")
    src = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")
    host = np.empty((n, 16), dtype=np.float32)
    flat_host = torch.from_numpy(np.empty((n, 16), dtype=np.float32))  # pageable, like a numpy array

    flat_dev = torch.empty((n, 16), dtype=torch.float32, device="cuda:0")

    def flat_dd():
        flat_dev.copy_(src)
        torch.cuda.synchronize()

    def flat_dh():
        flat_host.copy_(src)
        torch.cuda.synchronize()

    t_dev, t_flat = timed(lambda: ctx.read_triangles_into(dev)), timed(flat_dd)
    assert dev.cpu().numpy().tobytes() == tris.tobytes(), "the device read is not the caller's array"
    lines.append(row("read into device memory (row scatter through the permutation)", t_dev, nbytes=nbytes))
    lines.append(row("yardstick: flat device-to-device copy of the same bytes", t_flat, nbytes=nbytes))
    lines.append(f"{'':64s} the read takes {statistics.median(t_dev) / statistics.median(t_flat):.2f} x the flat copy")
    t_host, t_flat = timed(lambda: ctx.read_triangles_into(host)), timed(flat_dh)
    assert host.tobytes() == tris.tobytes(), "the host read is not the caller's array"
    lines.append(row("read into a host array (scatter into staging, one copy)", t_host, nbytes=nbytes))
    lines.append(row("yardstick: flat device-to-host copy into pageable memory", t_flat, nbytes=nbytes))
    lines.append(f"{'':64s} the read takes {statistics.median(t_host) / statistics.median(t_flat):.2f} x the flat copy")
    lines += ["", f"== RVPT_HIP_FORMAT_SURFACE_POINTS: {N} records per call =="]
    rng = np.random.RandomState(1)
    stored = ctx.surface_points(np.arange(8, dtype=np.uint32), 0.25, 0.25)  # (warms the inverse permutation)
    assert np.isfinite(stored["point"]).all()
    # "stored order": the caller's indices of consecutive stored rows, perm[s] for s = 0, 1, ... — the permutation of the same (deterministic) build, read back
    # from a laboratory context
    lab = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    assert lab.build_scene(tris, mats, "sah") == "sah"
    perm = lab.scene_state(["perm"])["perm"].reshape(-1).astype(np.uint32)
    lab.close()
    assert perm.shape[0] == n and np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint32))
    for order, prim in (("random prim", rng.randint(0, n, N).astype(np.uint32)), ("stored order", perm[np.arange(N) % n])):
        rec = np.zeros(N, dtype=native.SURFACE_POINT_DTYPE)
        rec["prim"], rec["u"], rec["v"] = prim, rng.uniform(0, 0.5, N), rng.uniform(0, 0.5, N)
        d = torch.from_numpy(rec.view(np.float32).reshape(-1, 12)).to("cuda:0")
        lines.append(row(f"surface_points, {order}, device records", timed(lambda: ctx.surface_points_into(d)), n=N))
        lines.append(row(f"surface_points, {order}, host records", timed(lambda: ctx.surface_points_into(rec)), n=N))
        got = d.cpu().numpy().view(native.SURFACE_POINT_DTYPE).reshape(-1)
        assert got.tobytes() == rec.tobytes(), "host and device records differ"
        k = rng.randint(0, N, 2000)
        want = scene.surface_points(tris, rec["prim"][k], rec["u"][k], rec["v"][k])
        assert want["point"].tobytes() == rec["point"][k].tobytes() and want["normal"].tobytes() == rec["normal"][k].tobytes(), "a sample of 2000 records differs from the statement"
    lines.append(f"{'':64s} host and device records equal byte for byte; 2000 sampled records of each order equal scene.surface_points")
    ctx.close()
    print("\n".join(lines), flush=True)
    write_section("\n".join(lines), resources=False)


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
    lines = [" (tools/bench_readback.py resources <parent tree>; tools/kernel_resources.py: the compiler's own metadata) ====", "",
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
    lines += table("the new kernel (rvpt_surface.hip; the row scatter is rvpt_refit.hip's carry_back_triangles, counted above)", tables(ROOT, ["rvpt_surface.hip"]))
    text = "\n".join(lines) + "\n"
    print(MARK + text)
    write_section(text, resources=True)
    return same


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rates"
    if mode == "resources":
        sys.exit(0 if resources(sys.argv[2]) else 1)
    rates()
