#!/usr/bin/env python3
"""Run on the GPU box: what it costs to get a finished frame out of the library — rvpt_hip_read into host memory (un-tile into the staging buffer, then a
device-to-host copy) against rvpt_hip_read into device memory of the same GPU (Context.read_into with a torch tensor: the un-tiling kernel writes the tensor, the
frame never visits the host), and against the floor of the host route, a bare device-to-host copy of the same byte count into pageable memory.  1920x1080 and
3840x2160, both formats, wall clock from the call to its return (both imply the wait), median of 20 on one box, the commit beside every row.  With a parent
library, its host read from the same run (a child process on RVPT_HIP_LIB) is the number the device read is set against.  -> stdout (profiles/device_frames.txt)
usage: tools/read_bench.py [--commit HASH] [--parent LIBRARY --parent-commit HASH] [--host-only]
One condition is asserted: the device RGBA32F read at 1920x1080 is below the flat-copy floor of the same 33 MB measured in this run."""
import argparse, os, statistics, subprocess, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from rvpt_amd import RenderSettings, native, scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", default=None)
ap.add_argument("--parent", default=None, help="the parent commit's librvpt_hip.so")
ap.add_argument("--parent-commit", default="parent")
ap.add_argument("--host-only", action="store_true", help="host reads only (what the child process on the parent library runs)")
args = ap.parse_args()
if args.commit is None:
    res = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
    args.commit = res.stdout.strip() if res.returncode == 0 and res.stdout.strip() else "unknown"

SIZES = [(1920, 1080), (3840, 2160)]
FORMATS = [("RGBA32F", native.FORMAT_RGBA32F, np.float32, 16), ("RGBA8", native.FORMAT_RGBA8_UNORM, np.uint8, 4)]
REPS = 20


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def row(what, size, fmt, nbytes, ts, commit):
    m = statistics.median(ts)
    print(f"{commit:>10s}  {size[0]:4d}x{size[1]:<4d} {fmt:8s} {what:44s} median {m * 1e3:8.3f} ms   min {min(ts) * 1e3:8.3f}   max {max(ts) * 1e3:8.3f}   n {len(ts)}   "
          f"{nbytes / 1e6:6.1f} MB  {nbytes / m / 1e9:8.1f} GB/s", flush=True)
    return m


import torch  # noqa: E402  (after rvpt_amd: native.load orders the runtimes)

tris, mats = scene.default_scene()
cam = np.zeros(20, np.float32)
cam[[0, 5, 10, 15]] = 1.0
medians = {}
for W, H in SIZES:
    cam[16], cam[17], cam[18] = W / H, np.radians(90.0), 4.0
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
    ctx.upload_scene(None, tris, mats)
    ctx.set_frame(RenderSettings(aa=1, current_frame=0).pack(), cam)
    ctx.dispatch()
    ctx.wait()
    for name, fmt, dt, px_bytes in FORMATS:
        nbytes = W * H * px_bytes
        host = np.empty((H, W, 4), dtype=dt)
        tag = args.parent_commit if args.host_only else args.commit
        medians[(W, name, "host")] = row("host read (un-tile + D2H copy, pageable)", (W, H), name, nbytes, timed(lambda: ctx.read_into(host, fmt)), tag)
        if args.host_only:
            continue
        dev = torch.empty((H, W, 4), dtype=torch.float32 if dt == np.float32 else torch.uint8, device="cuda:0")
        medians[(W, name, "device")] = row("device read (un-tile into the tensor)", (W, H), name, nbytes, timed(lambda: ctx.read_into(dev, fmt)), tag)
        assert dev.cpu().numpy().tobytes() == host.tobytes(), "the device read and the host read differ"
        view = torch.empty(W * H * 4 + 4, dtype=dev.dtype, device="cuda:0")[(1 if dt == np.float32 else 4):][: W * H * 4].view(H, W, 4)
        medians[(W, name, "device4")] = row("device read, destination 4-byte aligned only", (W, H), name, nbytes, timed(lambda: ctx.read_into(view, fmt)), tag)
        flat_src = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        flat_dst = torch.from_numpy(np.empty(nbytes, dtype=np.uint8))  # pageable, like a numpy array
        def flat():
            flat_dst.copy_(flat_src)
            torch.cuda.synchronize()
        medians[(W, name, "floor")] = row("floor: flat D2H copy of the same bytes", (W, H), name, nbytes, timed(flat), tag)
    ctx.close()

if args.host_only:
    sys.exit(0)

if args.parent:
    print(f"\n== the parent commit's host read, from this run (child process, RVPT_HIP_LIB={Path(args.parent).name} of {args.parent_commit}) ==", flush=True)
    res = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--host-only", "--parent-commit", args.parent_commit],
                         env={**os.environ, "RVPT_HIP_LIB": str(Path(args.parent).resolve()), "RVPT_HIP_QUIET": "1"}, capture_output=True, text=True, timeout=600)
    print(res.stdout, end="")
    if res.returncode != 0:
        raise SystemExit(f"the child on the parent library failed:\n{res.stderr[-2000:]}")

h, d, f = medians[(1920, "RGBA32F", "host")], medians[(1920, "RGBA32F", "device")], medians[(1920, "RGBA32F", "floor")]
print(f"\nsummary 1920x1080 RGBA32F ({args.commit}): device read {d * 1e3:.3f} ms, host read {h * 1e3:.3f} ms = {h / d:.1f} x, flat-copy floor {f * 1e3:.3f} ms = {f / d:.1f} x the device read; "
      f"stages of the host read: un-tile kernel + wait ~ {d * 1e3:.3f} ms (the device read is that stage alone), D2H copy ~ {(h - d) * 1e3:.3f} ms")
assert d < f, f"device RGBA32F read at 1920x1080 ({d * 1e3:.3f} ms) is not below the flat-copy floor of the same bytes ({f * 1e3:.3f} ms)"
print("assertion met: the device RGBA32F read at 1920x1080 is below the flat-copy floor of 33 MB measured in this run")
