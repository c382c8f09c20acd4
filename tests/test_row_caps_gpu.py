"""The row caps of the packet kernel's bounce rounds on the device (rvpt_vis.h: the row caps; rvpt_packets.hip: a uniform round whose rays all rise above their row's
cap walks nothing).  The laboratory build's RVPT_HIP_PACKETS_ROW_CAPS=0, read at upload_scene, fills every cap with +inf: the same kernel, which then never skips.
  * exact: image bytes, statistics (segments, samples) and the tile buffer are the same with the caps (the default) and with the knob at 0 — on the default scene
    (two image sizes, aa 1 and 2, float and UNORM8 accumulation, a listed launch in frame-run order), and on the default scene, the lifted-rim fan, the canopy and
    Cornell level 1 with their own materials, with every material a mirror (grazing reflections: dot(d, normal) near 0) and with every material glass (the
    refracting branch leaves on the other side);
  * superset: full paths from every pixel against EVERY triangle — no pair the float test accepts lies on a segment its row cap declares out of reach
    (rvpt_hip_selftest_bounce_cull out[7] == 0: refined row, row box and row cap together), on the same scenes and three poses each;
  * rvpt_hip_get_cull_info names the caps in bit 11: set by default, clear under the knob."""
import numpy as np
import pytest

import test_row_boxes_gpu as G
from test_row_boxes_gpu import FAN_POSES, LAUNCHES, native  # noqa: F401  (the fixture)
from test_row_boxes_tight_gpu import GRAZING
from test_row_caps import canopy
from test_sky_list import POSES

CAPS = "RVPT_HIP_PACKETS_ROW_CAPS"
KNOBS = ("RVPT_HIP_PACKETS_ROW_RULE", "RVPT_HIP_PACKETS_ROW_BOXES", "RVPT_HIP_PACKETS_BOX_CULL", CAPS)
CANOPY_POSES = [((0.3, 0.3, 1.5), (180.0, 0.0, 0.0), 90.0), ((0.4, 0.2, 0.15), (180.0, 0.0, 0.0), 120.0), ((-0.6, 0.3, 0.12), (100.0, 0.0, 0.0), 100.0)]  # above both, between them, beside them
NAMED = [POSES[k] for k in ("default", "bench", "oblique")]
SCENE_POSES = {"default": NAMED, "cornell1": NAMED, "lifted": [FAN_POSES[0], FAN_POSES[2], GRAZING], "canopy": CANOPY_POSES}


def scene_named(native, name, material):
    from rvpt_amd import scene
    from test_row_boxes_tight_gpu import scene_named as tight_scene_named
    if name == "canopy":
        tris, mats = scene.make_triangles(canopy(), 1), scene.default_materials()
    else:
        tris, mats = tight_scene_named(native, name)
    mats = mats.copy()
    if material == "mirror":
        mats[:, 8] = float(scene.MIRROR)
        mats[:, 0:3] = np.maximum(mats[:, 0:3], 0.8)
    elif material == "glass":
        mats[:, 8] = float(scene.DIELECTRIC)
        mats[:, 0:3] = np.maximum(mats[:, 0:3], 0.8)
        mats[:, 3] = 1.5
    return tris, mats


def render(native, monkeypatch, caps_on, tris, mats, W, H, launches, aa=1, flags=0):
    """launches: (pose as (translation, rotation, fov), first frame, frames, upload the scene again first).  Returns (image bytes, stats, tile buffer bytes, cull bits)."""
    import torch
    from rvpt_amd import Camera, RenderSettings
    from rvpt_amd.distributed import _DeviceBuffer
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if not caps_on:
        monkeypatch.setenv(CAPS, "0")
    monkeypatch.setenv("RVPT_HIP_PACKETS_SKY_LIST", "2")  # (a batched launch of four frames or more takes the listed path at once)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE | native.COUNT_SEGMENTS | flags, lab=True)
    try:
        ctx.upload_scene(None, tris, mats)
        info = []
        for (tr, rot, fov), first, n, reupload in launches:
            if reupload:
                ctx.upload_scene(None, tris, mats)
            c = Camera(W / H)
            c.translation, c.rotation, c.fov = np.array(tr, float), np.array(rot, float), fov
            ctx.set_frame(RenderSettings(aa=aa, current_frame=first).pack(), c.get_data())
            ctx.dispatch() if n == 1 else ctx.dispatch_frames(n)
            info.append(ctx.cull_info())
        ctx.wait()
        ptr, _, slot_bytes = ctx.tile_buffer()
        torch.cuda.synchronize()
        tiles = torch.as_tensor(_DeviceBuffer(ptr, slot_bytes // 4), device="cuda:0").cpu().numpy().copy()
        return ctx.read().view(np.uint32).copy(), tuple(ctx.stats()), tiles.view(np.uint32), info
    finally:
        ctx.close()
        monkeypatch.delenv(CAPS, raising=False)


def same(native, monkeypatch, tris, mats, W, H, launches, **kw):
    img, st, tiles, info = render(native, monkeypatch, True, tris, mats, W, H, launches, **kw)
    assert all(i & native.CULL_ROW_BOXES and i & native.CULL_ROW_CAPS for i in info), [hex(i) for i in info]
    assert img.any() and st[0] > st[1] > 0  # (bounce segments were traced)
    img2, st2, tiles2, info2 = render(native, monkeypatch, False, tris, mats, W, H, launches, **kw)
    assert all(i & native.CULL_ROW_BOXES and not i & native.CULL_ROW_CAPS for i in info2), [hex(i) for i in info2]
    assert [i & ~native.CULL_ROW_CAPS for i in info] == info2  # (nothing else about the launches differs)
    assert st2 == st, (st2, st)
    assert np.array_equal(img2, img)
    assert np.array_equal(tiles2, tiles)
    return info


def named_launches(launches):
    return [(POSES[pose], first, n, re) for pose, first, n, re in launches]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(96, 64), (100, 52)])
@pytest.mark.parametrize("aa", [1, 2])
def test_row_caps_are_exact(native, monkeypatch, W, H, aa):
    tris, mats = scene_named(native, "default", "own")
    same(native, monkeypatch, tris, mats, W, H, named_launches(LAUNCHES), aa=aa)


@pytest.mark.gpu
def test_row_caps_are_exact_with_unorm8_accumulation(native, monkeypatch):
    tris, mats = scene_named(native, "default", "own")
    same(native, monkeypatch, tris, mats, 96, 64, named_launches(LAUNCHES[:4]), flags=native.ACCUM_UNORM8)


@pytest.mark.gpu
def test_row_caps_are_exact_on_the_listed_path_with_frame_runs(native, monkeypatch):
    """(a 20-frame launch at 640 x 360 takes the listed instance in frame-run order: the headline's kernel)"""
    tris, mats = scene_named(native, "default", "own")
    info = same(native, monkeypatch, tris, mats, 640, 360, [(POSES["default"], 0, 20, False)])
    assert info[0] & native.CULL_SKY_LIST and info[0] & native.CULL_FRAME_RUNS, info


@pytest.mark.gpu
@pytest.mark.parametrize("material", ["own", "mirror", "glass"])
@pytest.mark.parametrize("name", ["default", "lifted", "canopy", "cornell1"])
def test_row_caps_are_exact_on_every_scene_and_material(native, monkeypatch, name, material):
    """one frame, a 3-frame launch, a 5-frame launch (the listed path) at the scene's first pose, then the other two poses, one after an upload; both image sizes,
    the second with aa 2"""
    tris, mats = scene_named(native, name, material)
    p = SCENE_POSES[name]
    launches = [(p[0], 0, 1, False), (p[0], 1, 3, False), (p[0], 4, 5, False), (p[1], 0, 5, False), (p[2], 5, 3, True)]
    same(native, monkeypatch, tris, mats, 96, 64, launches)
    same(native, monkeypatch, tris, mats, 100, 52, launches[2:], aa=2)


@pytest.mark.gpu
@pytest.mark.parametrize("material", ["own", "mirror", "glass"])
@pytest.mark.parametrize("name", ["default", "lifted", "canopy", "cornell1"])
def test_row_caps_never_declare_an_accepted_hit_out_of_reach(native, monkeypatch, name, material):
    from rvpt_amd import Camera, RenderSettings
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    W, H = 128, 72
    tris, mats = scene_named(native, name, material)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE, lab=True)
    try:
        ctx.upload_scene(None, tris, mats)
        total = 0
        for tr, rot, fov in SCENE_POSES[name]:
            c = Camera(W / H)
            c.translation, c.rotation, c.fov = np.array(tr, float), np.array(rot, float), fov
            ctx.set_frame(RenderSettings(aa=1, current_frame=3).pack(), c.get_data())
            ctx.dispatch()  # (which tables the context holds: the launch's cull word)
            ctx.wait()
            assert ctx.cull_info() & native.CULL_ROW_BOXES and ctx.cull_info() & native.CULL_ROW_CAPS, hex(ctx.cull_info())
            out = ctx.selftest_bounce_cull(2)
            print(name, material, tr, out)
            assert out[1] == 0 and out[4] == 0 and out[7] == 0, (name, material, tr, out)
            total += out[0]
        if name in ("default", "cornell1"):  # (nothing rises far over the fan, and the canopy's two triangles see each other from one side only)
            assert total > 0
    finally:
        ctx.close()
