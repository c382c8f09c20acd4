"""The row boxes of the packet kernel's bounce rounds on the device (rvpt_vis.h, rvpt_packets.hip: a packet whose rays all leave one triangle walks that row's
refined words and its own boxes; every other packet the union of rows and the shared leaf boxes):
  * superset: full paths from every pixel against EVERY triangle — a pair the float test accepts on a segment that leaves a triangle is in the refined row of where it
    leaves from and passes that row's box of its leaf (rvpt_hip_selftest_bounce_cull out[7] == 0, beside the table's out[1] and the leaf boxes' out[4]);
  * exact: image bytes, statistics and the tile buffer are the same with the row boxes (the default), with RVPT_HIP_PACKETS_BOX_CULL=0 (row boxes off together with
    the leaf boxes) and with the laboratory knob RVPT_HIP_PACKETS_ROW_BOXES=0 (row boxes alone off);
  * both paths run somewhere in these scenes (the instrumented build's timeline, tools/row_box_paths.py)."""
import json
import subprocess
import sys

import numpy as np
import pytest

from _util import ROOT, scene_by_name
from test_row_boxes import bump_fan
from test_sky_list import POSES, camera

KNOBS = {"on": {}, "box_cull_off": {"RVPT_HIP_PACKETS_BOX_CULL": "0"}, "row_boxes_off": {"RVPT_HIP_PACKETS_ROW_BOXES": "0"}}


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def scene_named(native, name):
    from rvpt_amd import scene
    if name in ("default", "showcase"):
        tris, mats, _ = scene_by_name(name)
        return tris, mats
    if name == "cornell1":
        tris, mats = scene.cornell_scene(1)
    elif name == "subdivided":  # 572 triangles, still resident in LDS: the rays of a packet leave many triangles
        tris, mats = scene.make_triangles(scene.subdivide(scene.default_model_positions(), 1), 1), scene.default_materials()
    else:  # the bump fan, seen from above (+z)
        tris, mats = scene.make_triangles(bump_fan(), 1), scene.default_materials()
    _, idx = native.build_bvh(tris)
    return tris[idx], mats


FAN_POSES = [((0, 0, 1.5), (180.0, 0, 0), 90.0), ((0.4, -0.3, 0.6), (195.0, 15.0, 0.0), 100.0), ((-0.8, 0.2, 0.3), (120.0, -10.0, 5.0), 110.0)]  # (the camera looks along +z: turned to look down at the fan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "showcase", "cornell1", "fan"])
def test_row_boxes_never_exclude_an_accepted_hit(native, name):
    from rvpt_amd import Camera, RenderSettings
    W, H = 128, 72
    tris, mats = scene_named(native, name)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE, lab=True)
    try:
        ctx.upload_scene(None, tris, mats)
        total = 0
        for tr, rot, fov in (FAN_POSES if name == "fan" else [POSES[k] for k in ("default", "bench", "oblique")]):
            c = Camera(W / H)
            c.translation, c.rotation, c.fov = np.array(tr, float), np.array(rot, float), fov
            ctx.set_frame(RenderSettings(aa=1, current_frame=3).pack(), c.get_data())
            out = ctx.selftest_bounce_cull(2)
            print(name, tr, out)
            assert out[1] == 0 and out[4] == 0 and out[7] == 0, (name, tr, out)
            total += out[0]
        if name != "fan":  # (nothing rises far enough over the fan to be hit from it: its accepted pairs may be none)
            assert total > 0
    finally:
        ctx.close()


def render(native, monkeypatch, knobs, name, W, H, launches, aa=1, flags=0):
    """launches: (pose, first frame, frames, upload the scene again first).  Returns (image bytes, stats, tile buffer bytes, cull bits per launch)."""
    import torch
    from rvpt_amd import RenderSettings
    from rvpt_amd.distributed import _DeviceBuffer
    for k in ("RVPT_HIP_PACKETS_BOX_CULL", "RVPT_HIP_PACKETS_ROW_BOXES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RVPT_HIP_PACKETS_SKY_LIST", "2")  # (a batched launch of four frames or more takes the listed path at once)
    tris, mats = scene_named(native, name)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE | native.COUNT_SEGMENTS | flags, lab=True)
    try:
        ctx.upload_scene(None, tris, mats)
        info = []
        for pose, first, n, reupload in launches:
            if reupload:
                ctx.upload_scene(None, tris, mats)
            ctx.set_frame(RenderSettings(aa=aa, current_frame=first).pack(), camera(W, H, pose))
            ctx.dispatch() if n == 1 else ctx.dispatch_frames(n)
            info.append(ctx.cull_info())
        ctx.wait()
        ptr, _, slot_bytes = ctx.tile_buffer()
        torch.cuda.synchronize()
        tiles = torch.as_tensor(_DeviceBuffer(ptr, slot_bytes // 4), device="cuda:0").cpu().numpy().copy()
        return ctx.read().view(np.uint32).copy(), tuple(ctx.stats()), tiles.view(np.uint32), info
    finally:
        ctx.close()


def same(native, monkeypatch, name, W, H, launches, **kw):
    img, st, tiles, info = render(native, monkeypatch, KNOBS["on"], name, W, H, launches, **kw)
    assert all(i & native.CULL_ROW_BOXES for i in info), info
    assert img.any() and st[0] > st[1] > 0  # (bounce segments were traced)
    for tag in ("box_cull_off", "row_boxes_off"):
        img2, st2, tiles2, info2 = render(native, monkeypatch, KNOBS[tag], name, W, H, launches, **kw)
        assert not any(i & native.CULL_ROW_BOXES for i in info2), (tag, info2)
        assert st2 == st, (tag, st2, st)
        assert np.array_equal(img2, img), tag
        assert np.array_equal(tiles2, tiles), tag
    return info


# one frame, a 3-frame launch, a 5-frame launch (the listed path), a camera move, a scene uploaded again
LAUNCHES = [("default", 0, 1, False), ("default", 1, 3, False), ("default", 4, 5, False), ("bench", 0, 5, False), ("bench", 5, 1, True), ("oblique", 0, 3, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(96, 64), (100, 52)])
@pytest.mark.parametrize("aa", [1, 2])
def test_row_boxes_are_exact(native, monkeypatch, W, H, aa):
    same(native, monkeypatch, "default", W, H, LAUNCHES, aa=aa)


@pytest.mark.gpu
def test_row_boxes_are_exact_on_the_listed_path(native, monkeypatch):
    """(images this small leave the listed instance no whole-block chunks: a 5-frame and a 20-frame launch at 640 x 360 take it)"""
    info = same(native, monkeypatch, "default", 640, 360, [("default", 0, 5, False), ("default", 5, 20, False), ("bench", 0, 5, False)])
    assert info[0] & native.CULL_SKY_LIST and info[1] & native.CULL_SKY_LIST, info


@pytest.mark.gpu
def test_row_boxes_are_exact_with_unorm8_accumulation(native, monkeypatch):
    same(native, monkeypatch, "default", 96, 64, LAUNCHES[:4], flags=native.ACCUM_UNORM8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["subdivided", "showcase"])
def test_row_boxes_are_exact_on_mixed_packets(native, monkeypatch, name):
    same(native, monkeypatch, name, 96, 64, LAUNCHES[:4])


@pytest.mark.gpu
def test_both_paths_of_the_bounce_rounds_are_taken():
    """The instrumented build's timeline over two of the launches above: the default scene's packets leave one triangle (row boxes), the subdivided model's
    leave many (union of rows, shared leaf boxes) — without both, the exactness tests above would say nothing about one of them."""
    got = {}
    for name in ("default", "subdivided"):
        res = subprocess.run([sys.executable, str(ROOT / "tools" / "row_box_paths.py"), name, "96", "64", "5"], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        got[name] = json.loads(res.stdout.strip().splitlines()[-1])
        print(got[name])
        assert got[name]["bounce_rounds"] > 0 and got[name]["cull_info"] & 0x100
    assert sum(g["row_box_rounds"] for g in got.values()) > 0
    assert sum(g["union_rounds"] for g in got.values()) > 0
