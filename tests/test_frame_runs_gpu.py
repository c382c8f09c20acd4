"""Listed launches in frame-run order (rvpt_packets.h: ListedWork, listed_item; rvpt_packets.hip: the run header): a block's frames follow each other in groups of
16 (the default) or of RVPT_HIP_PACKETS_FRAME_RUNS frames and the wave makes the block's origin, the pixels' hash and the candidate ballots once per run.  RVPT_HIP_PACKETS_FRAME_RUNS=0 keeps the frame-major order with
the set-up of every round: the same accumulator bytes, tile buffer and statistics, and rvpt_hip_get_cull_info tells which of the two ran.  The default takes the
run order for launches of 16 frames or more (rvpt_abi.hip: choose_launch); RVPT_HIP_PACKETS_FRAME_RUNS=8 takes it for every listed launch, so each case is
rendered three times: knob 0, the default and knob 8.

Images of a few thousand pixels leave the listed instance no whole-block chunks under the default work plan, so the small cases ride with the laboratory knobs
RVPT_HIP_FIRST_UNITS=4 and RVPT_HIP_CLAIM_UNITS=4 — chunks of ONE block, which cut every run between two of its frames; 640 x 360 takes the default plan
(128-item static chunks, 512-item claims)."""
import numpy as np
import pytest

from test_row_boxes_gpu import scene_named
from test_sky_list import camera

ONE_BLOCK_CHUNKS = {"RVPT_HIP_FIRST_UNITS": "4", "RVPT_HIP_CLAIM_UNITS": "4"}


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def render(native, monkeypatch, runs, name, W, H, launches, plan, flags=0):
    """launches: (pose, first frame, frames).  Returns (image bytes, stats, tile buffer bytes, cull bits per launch)."""
    import torch
    from rvpt_amd import RenderSettings
    from rvpt_amd.distributed import _DeviceBuffer
    for k in ("RVPT_HIP_PACKETS_FRAME_RUNS", *ONE_BLOCK_CHUNKS):
        monkeypatch.delenv(k, raising=False)
    if runs is not None:
        monkeypatch.setenv("RVPT_HIP_PACKETS_FRAME_RUNS", runs)
    for k, v in plan.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("RVPT_HIP_PACKETS_SKY_LIST", "2")  # (a batched launch of four frames or more takes the listed path at once)
    tris, mats = scene_named(native, name)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE | native.COUNT_SEGMENTS | flags, lab=True)
    try:
        ctx.upload_scene(None, tris, mats)
        info = []
        for pose, first, n in launches:
            ctx.set_frame(RenderSettings(aa=1, current_frame=first).pack(), camera(W, H, pose))
            ctx.dispatch_frames(n)
            info.append(ctx.cull_info())
        ctx.wait()
        ptr, _, slot_bytes = ctx.tile_buffer()
        torch.cuda.synchronize()
        tiles = torch.as_tensor(_DeviceBuffer(ptr, slot_bytes // 4), device="cuda:0").cpu().numpy().copy()
        return ctx.read().view(np.uint32).copy(), tuple(ctx.stats()), tiles.view(np.uint32), info
    finally:
        ctx.close()


def same(native, monkeypatch, name, W, H, launches, plan=ONE_BLOCK_CHUNKS, **kw):
    img0, st0, tiles0, info0 = render(native, monkeypatch, "0", name, W, H, launches, plan, **kw)
    assert all(i & native.CULL_SKY_LIST and not i & native.CULL_FRAME_RUNS for i in info0), info0  # every launch here is listed; knob 0: never in run order
    assert img0.any() and st0[0] > st0[1] > 0  # (bounce segments were traced)
    for knob in (None, "8"):
        img, st, tiles, info = render(native, monkeypatch, knob, name, W, H, launches, plan, **kw)
        print(name, W, H, launches, "knob", knob, "stats", st, "cull info", [hex(i) for i in info])
        assert all(i & native.CULL_SKY_LIST for i in info), info
        # the new path is reported as taken: by every launch with the knob, by the launches of two whole groups or more without it
        assert [bool(i & native.CULL_FRAME_RUNS) for i in info] == [knob is not None or n >= 16 for _, _, n in launches], (knob, info)
        assert st == st0, (knob, st, st0)
        assert np.array_equal(img, img0), knob
        assert np.array_equal(tiles, tiles0), knob


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(96, 64), (100, 52)])
@pytest.mark.parametrize("n", [4, 9, 20, 64])
def test_frame_runs_are_exact(native, monkeypatch, W, H, n):
    # with the knob at 8: a lone short group, 8 + 1, 8 + 8 + 4, whole groups; the default takes 20 as 16 + 4 and 64 as 4 x 16; from frame 0 and, chained, from a later frame (5 frames: a lone group of another length)
    same(native, monkeypatch, "default", W, H, [("default", 0, n), ("default", n, 5), ("bench", 3, n)])


@pytest.mark.gpu
def test_frame_runs_are_exact_where_chunks_cut_runs(native, monkeypatch):
    # the default work plan: 128-item static chunks (two frames of a run) and 512-item claims that start wherever the static part ends
    same(native, monkeypatch, "default", 640, 360, [("default", 0, 9), ("default", 9, 9)], plan={})


@pytest.mark.gpu
def test_frame_runs_are_exact_beyond_192_triangles(native, monkeypatch):
    # 572 triangles: the header keeps no ballots, every round scans the rectangles
    same(native, monkeypatch, "subdivided", 100, 52, [("default", 0, 20), ("oblique", 20, 9)])


@pytest.mark.gpu
def test_frame_runs_are_exact_with_unorm8_accumulation(native, monkeypatch):
    same(native, monkeypatch, "default", 96, 64, [("default", 0, 20), ("default", 20, 6)], flags=native.ACCUM_UNORM8)
