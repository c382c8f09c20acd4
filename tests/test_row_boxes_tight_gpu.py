"""The tight rule of the row boxes on the device (rvpt_vis.h: kRowRuleTight — the tables every upload_scene makes; the laboratory build's
RVPT_HIP_PACKETS_ROW_RULE=0, read at upload_scene, makes round 8's instead):
  * superset: full paths from every pixel against EVERY triangle — a pair the float test accepts on a segment that leaves a triangle is in the tight refined row of
    where it leaves from and passes that row's tight box of its leaf (rvpt_hip_selftest_bounce_cull out[7] == 0, beside the table's out[1] and the leaf boxes'
    out[4]), with the scenes' own materials and with every material a mirror: mirror bounces under a grazing camera run along the coplanar neighbours, an EPSILON
    over their plane, which is where an H0 set too high would show;
  * exact: image bytes, statistics (segments, samples) and the tile buffer are the same with the tight tables (the default), with round 8's
    (RVPT_HIP_PACKETS_ROW_RULE=0) and without row boxes (RVPT_HIP_PACKETS_ROW_BOXES=0); rvpt_hip_get_cull_info names the rule in bit 10."""
import numpy as np
import pytest

import test_row_boxes_gpu as G
from test_row_boxes_gpu import FAN_POSES, LAUNCHES, native  # noqa: F401  (the fixture)
from test_row_boxes_tight import lifted_rim_fan
from test_sky_list import POSES

RULE = "RVPT_HIP_PACKETS_ROW_RULE"
GRAZING = ((0.0, 0.0, 0.06), (95.0, 0.0, 0.0), 100.0)  # just over the fans' centre, looking along their plane and a little down


def scene_named(native, name):
    from rvpt_amd import scene
    if name != "lifted":
        return G.scene_named(native, name)
    tris, mats = scene.make_triangles(lifted_rim_fan(), 1), scene.default_materials()
    _, idx = native.build_bvh(tris)
    return tris[idx], mats


@pytest.mark.gpu
@pytest.mark.parametrize("material", ["own", "mirror"])
@pytest.mark.parametrize("name", ["default", "showcase", "cornell1", "fan", "lifted"])
def test_tight_row_boxes_never_exclude_an_accepted_hit(native, monkeypatch, name, material):
    from rvpt_amd import Camera, RenderSettings, scene
    monkeypatch.delenv(RULE, raising=False)
    monkeypatch.delenv("RVPT_HIP_PACKETS_ROW_BOXES", raising=False)
    monkeypatch.delenv("RVPT_HIP_PACKETS_BOX_CULL", raising=False)
    W, H = 128, 72
    tris, mats = scene_named(native, name)
    if material == "mirror":
        mats = mats.copy()
        mats[:, 8] = float(scene.MIRROR)
        mats[:, 0:3] = np.maximum(mats[:, 0:3], 0.8)  # (a black mirror ends no path early, but keep the paths alive in any case)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE, lab=True)
    try:
        ctx.upload_scene(None, tris, mats)
        total = 0
        poses = [FAN_POSES[0], FAN_POSES[2], GRAZING] if name in ("fan", "lifted") else [POSES[k] for k in ("default", "bench", "oblique")]
        for tr, rot, fov in poses:
            c = Camera(W / H)
            c.translation, c.rotation, c.fov = np.array(tr, float), np.array(rot, float), fov
            ctx.set_frame(RenderSettings(aa=1, current_frame=3).pack(), c.get_data())
            ctx.dispatch()  # (which tables the context holds: the launch's cull word)
            ctx.wait()
            assert ctx.cull_info() & native.CULL_ROW_BOXES and ctx.cull_info() & native.CULL_ROW_RULE_TIGHT, hex(ctx.cull_info())
            out = ctx.selftest_bounce_cull(2)
            print(name, material, tr, out)
            assert out[1] == 0 and out[4] == 0 and out[7] == 0, (name, material, tr, out)
            total += out[0]
        if name not in ("fan", "lifted"):  # (nothing rises far over the fans: their accepted pairs may be none)
            assert total > 0
    finally:
        ctx.close()


def same(native, monkeypatch, name, W, H, launches, **kw):
    monkeypatch.delenv(RULE, raising=False)
    img, st, tiles, info = G.render(native, monkeypatch, {}, name, W, H, launches, **kw)
    assert all(i & native.CULL_ROW_BOXES and i & native.CULL_ROW_RULE_TIGHT for i in info), info
    assert img.any() and st[0] > st[1] > 0  # (bounce segments were traced)
    for tag, knobs in (("row_rule_0", {RULE: "0"}), ("row_boxes_off", {"RVPT_HIP_PACKETS_ROW_BOXES": "0"})):
        monkeypatch.delenv(RULE, raising=False)
        img2, st2, tiles2, info2 = G.render(native, monkeypatch, knobs, name, W, H, launches, **kw)
        assert not any(i & native.CULL_ROW_RULE_TIGHT for i in info2) and all(bool(i & native.CULL_ROW_BOXES) == (tag == "row_rule_0") for i in info2), (tag, info2)
        assert st2 == st, (tag, st2, st)
        assert np.array_equal(img2, img), tag
        assert np.array_equal(tiles2, tiles), tag
    monkeypatch.delenv(RULE, raising=False)
    return info


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(96, 64), (100, 52)])
@pytest.mark.parametrize("aa", [1, 2])
def test_tight_row_boxes_are_exact(native, monkeypatch, W, H, aa):
    same(native, monkeypatch, "default", W, H, LAUNCHES, aa=aa)


@pytest.mark.gpu
def test_tight_row_boxes_are_exact_with_unorm8_accumulation(native, monkeypatch):
    same(native, monkeypatch, "default", 96, 64, LAUNCHES[:4], flags=native.ACCUM_UNORM8)


@pytest.mark.gpu
def test_tight_row_boxes_are_exact_on_the_listed_path_with_frame_runs(native, monkeypatch):
    """(a 20-frame launch at 640 x 360 takes the listed instance in frame-run order)"""
    info = same(native, monkeypatch, "default", 640, 360, [("default", 0, 20, False)])
    assert info[0] & native.CULL_SKY_LIST and info[0] & native.CULL_FRAME_RUNS, info


@pytest.mark.gpu
def test_tight_row_boxes_are_exact_on_the_subdivided_model(native, monkeypatch):
    same(native, monkeypatch, "subdivided", 96, 64, LAUNCHES[:4])
