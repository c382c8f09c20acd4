#!/usr/bin/env python3
"""Run on a GPU: which path the culled bounce rounds of ONE packet-kernel launch took — the row boxes (every ray of the packet leaves one triangle on one side)
or the union of rows with the shared leaf boxes — and how many triangles they walked, from the per-wave timeline of the instrumented laboratory build
(rvpt_amd/build.py: build_native_timeline; rvpt_packets.hip: t[3] rounds, t[5] triangles walked | rounds on the row boxes << 32).
usage: tools/row_box_paths.py <default|subdivided|showcase|cornell1> <width> <height> <frames in the launch>   -> one JSON line"""
import json, os, sys, tempfile
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
name, W, H, frames = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
from rvpt_amd import build as B
os.environ["RVPT_HIP_LAB_LIB"] = str(B.build_native_timeline())
out = Path(tempfile.mkdtemp()) / "timeline.bin"
os.environ["RVPT_HIP_TIMELINE"] = str(out)
os.environ["RVPT_HIP_PACKETS_SKY_LIST"] = "2"  # (a batched launch takes the listed path at once)
import numpy as np
from rvpt_amd import Camera, RenderSettings, native, scene


def make(name):
    if name == "subdivided":  # the default model, every triangle split in four: 572 triangles, still resident in LDS; a packet's rays leave many of them
        tris, mats = scene.make_triangles(scene.subdivide(scene.default_model_positions(), 1), 1), scene.default_materials()
    elif name == "cornell1":
        tris, mats = scene.cornell_scene(1)
    else:
        tris, mats = {"default": scene.default_scene, "showcase": scene.materials_showcase_scene}[name]()
    _, idx = native.build_bvh(tris)
    return tris[idx], mats


tris, mats = make(name)
ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE, lab=True)
try:
    ctx.upload_scene(None, tris, mats)
    ctx.set_frame(RenderSettings(aa=1, current_frame=0).pack(), Camera(W / H).get_data())
    ctx.dispatch() if frames == 1 else ctx.dispatch_frames(frames)
    ctx.wait()
    info, grid = ctx.cull_info(), ctx.launch_info()[0]
finally:
    ctx.close()  # (writes the timeline)
raw = np.fromfile(out, dtype=np.uint64).reshape(-1, 8)[: grid * 4]
bounce = int((raw[:, 3] >> np.uint64(32)).sum())
uniform = int((raw[:, 5] >> np.uint64(32)).sum())
walked = int((raw[:, 5] & np.uint64(0xFFFFFFFF)).sum())
print(json.dumps({"scene": name, "triangles": int(len(tris)), "width": W, "height": H, "frames": frames, "cull_info": info, "bounce_rounds": bounce, "row_box_rounds": uniform,
                  "union_rounds": bounce - uniform, "triangles_walked": walked, "walked_per_round": walked / max(1, bounce)}))
