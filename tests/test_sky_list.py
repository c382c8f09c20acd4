"""Batched packet-kernel launches that claim only the blocks that are not SKY (rvpt_packets.hip: sky_blocks, the LISTED instance) and blend the sky from the RNG
(rvpt_kernels.hip: blend_accumulate_sky): the same image bytes, the same statistics and the same tile buffer, padding included, as the path that traces every
block (RVPT_HIP_PACKETS_SKY_LIST=0 against =2, which waits for the list on first use so that the first batched launch already takes it; a knob of the
laboratory build, whose packet kernels are the release build's)."""
import numpy as np
import pytest

from _util import scene_by_name

# the poses of tests/golden/default_{default,bench,oblique}_*: (translation, rotation, vertical field of view)
POSES = {"default": ((0, 0, 0), (0, 0, 0), 90.0), "bench": ((0, 0.9, -2.5), (0, 0, 0), 90.0), "oblique": ((1.4, 1.6, -1.2), (-40.0, 25.0, 10.0), 70.0)}


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def camera(W, H, pose):
    from rvpt_amd import Camera
    tr, rot, fov = POSES[pose]
    c = Camera(W / H)
    c.translation, c.rotation, c.fov = np.array(tr, float), np.array(rot, float), fov
    return c.get_data()


def render(native, monkeypatch, knob, W, H, launches, world=1, rank=0, flags=0):
    """launches: (pose, first frame, frames, max_bounces, upload the scene again first).  Returns (image bytes, stats, tile buffer bytes, cull bits per launch)."""
    import torch
    from rvpt_amd import RenderSettings
    from rvpt_amd.distributed import _DeviceBuffer
    monkeypatch.setenv("RVPT_HIP_PACKETS_SKY_LIST", str(knob))
    tris, mats, _ = scene_by_name("default")
    ctx = native.Context(W, H, 0, rank, world, native.TRAVERSAL_BRUTE | native.COUNT_SEGMENTS | flags, lab=True)
    try:
        ctx.upload_scene(None, tris, mats)
        info = []
        for pose, first, n, bounces, reupload in launches:
            if reupload:
                ctx.upload_scene(None, tris, mats)
            ctx.set_frame(RenderSettings(aa=1, current_frame=first, max_bounces=bounces).pack(), camera(W, H, pose))
            ctx.dispatch_frames(n)
            info.append(ctx.cull_info())
        ctx.wait()
        ptr, _, slot_bytes = ctx.tile_buffer()
        torch.cuda.synchronize()
        tiles = torch.as_tensor(_DeviceBuffer(ptr, slot_bytes // 4), device="cuda:0").cpu().numpy().copy()
        return ctx.read().view(np.uint32).copy(), tuple(ctx.stats()), tiles.view(np.uint32), info
    finally:
        ctx.close()


def same(native, monkeypatch, W, H, launches, listed, **kw):
    img0, st0, tiles0, info0 = render(native, monkeypatch, 0, W, H, launches, **kw)
    img2, st2, tiles2, info2 = render(native, monkeypatch, 2, W, H, launches, **kw)
    assert not any(i & native.CULL_SKY_LIST for i in info0)  # knob 0: never the listed path
    assert [bool(i & native.CULL_SKY_LIST) if want is not None else None for i, want in zip(info2, listed)] == listed, info2  # (None: either; a pose may leave no sky)
    assert st2 == st0
    assert np.array_equal(img2, img0)
    assert np.array_equal(tiles2, tiles0)
    return img0


@pytest.mark.gpu
@pytest.mark.parametrize("pose", ["default", "bench", "oblique"])
def test_sky_list_is_exact_at_the_golden_poses(native, monkeypatch, pose):
    img = same(native, monkeypatch, 1920, 1080, [(pose, 0, 20, 8, False), (pose, 20, 4, 8, False)], [True, True])
    assert img.any()


@pytest.mark.gpu
def test_sky_list_is_exact_over_launch_sizes_and_chains(native, monkeypatch):
    # 4, 20 and 64 frames; chains that accumulate over several launches (frame0 != 0); a launch below four frames keeps the old path
    same(native, monkeypatch, 1920, 1080, [("default", 0, 4, 8, False), ("default", 4, 64, 8, False), ("default", 68, 2, 8, False), ("default", 70, 20, 8, False)],
         [True, True, False, True])


@pytest.mark.gpu
def test_sky_list_is_exact_with_unorm8_accumulation(native, monkeypatch):
    same(native, monkeypatch, 1920, 1080, [("default", 0, 20, 8, False), ("default", 20, 6, 8, False)], [True, True], flags=native.ACCUM_UNORM8)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(1000, 563), (640, 360)])
def test_sky_list_is_exact_with_partial_edge_tiles(native, monkeypatch, W, H):
    same(native, monkeypatch, W, H, [("default", 0, 20, 8, False), ("oblique", 0, 5, 8, False)], [True, None])


@pytest.mark.gpu
@pytest.mark.parametrize("world,rank", [(8, 3), (3, 1)])
def test_sky_list_is_exact_on_a_share(native, monkeypatch, world, rank):
    same(native, monkeypatch, 1920, 1080, [("default", 0, 20, 8, False), ("default", 20, 20, 8, False)], [True, True], world=world, rank=rank)


@pytest.mark.gpu
def test_sky_list_follows_the_camera_and_the_scene(native, monkeypatch):
    # a camera moved between launches (the slot's list is made again), a scene uploaded again (the same), max_bounces 1; max_bounces 0 never runs the packet kernel
    same(native, monkeypatch, 1920, 1080, [("default", 0, 20, 8, False), ("bench", 0, 20, 8, False), ("bench", 20, 8, 8, True), ("oblique", 0, 4, 1, False),
                                           ("oblique", 4, 4, 0, False), ("default", 0, 20, 8, False)],
         [True, True, True, True, False, True])


@pytest.mark.gpu
def test_release_library_takes_the_listed_path_once_the_list_has_arrived(native, monkeypatch):
    """The release build (the knob's default: the listed path once the slot's list is on the host, never waited for) against the laboratory build with the
    knob off: 20-frame launches at one camera, one per slot of the rotation, then, after a wait, one more on the first slot — same bytes, statistics and tile buffer."""
    import torch
    from rvpt_amd import RenderSettings
    from rvpt_amd.distributed import _DeviceBuffer
    tris, mats, _ = scene_by_name("default")
    W, H = 1920, 1080
    out = []
    for lab, knob in ((False, None), (True, "0")):
        if knob is None:
            monkeypatch.delenv("RVPT_HIP_PACKETS_SKY_LIST", raising=False)
        else:
            monkeypatch.setenv("RVPT_HIP_PACKETS_SKY_LIST", knob)
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE | native.COUNT_SEGMENTS, lab=lab)
        try:
            ctx.upload_scene(None, tris, mats)
            info = []
            # one launch on every slot of the rotation, a wait (every slot's list has arrived), then the next launch: the first slot again
            ctx.set_frame(RenderSettings(aa=1, current_frame=0).pack(), camera(W, H, "default"))
            ctx.dispatch_frames(20)
            info.append(ctx.cull_info())
            slots = ctx.launch_info()[3]
            for k in range(1, slots + 1):
                if k == slots:
                    ctx.wait()
                ctx.set_frame(RenderSettings(aa=1, current_frame=20 * k).pack(), camera(W, H, "default"))
                ctx.dispatch_frames(20)
                info.append(ctx.cull_info())
            ctx.wait()
            ptr, _, slot_bytes = ctx.tile_buffer()
            torch.cuda.synchronize()
            tiles = torch.as_tensor(_DeviceBuffer(ptr, slot_bytes // 4), device="cuda:0").cpu().numpy().view(np.uint32).copy()
            out.append((ctx.read().view(np.uint32).copy(), tuple(ctx.stats()), tiles, info))
        finally:
            ctx.close()
    (img1, st1, tiles1, info1), (img0, st0, tiles0, info0) = out
    assert not info1[0] & native.CULL_SKY_LIST and not any(i & native.CULL_SKY_LIST for i in info0)  # a first launch at a camera never waits for its list
    assert info1[-1] & native.CULL_SKY_LIST  # the last launch reuses the first one's slot, whose list has arrived
    assert st1 == st0 and np.array_equal(img1, img0) and np.array_equal(tiles1, tiles0)
