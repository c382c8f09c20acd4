"""Frames that stay on the device: rvpt_hip_read into, and rvpt_hip_write_accum from, device memory of the context's GPU (Context.read_into, Context.write_accum
with a tensor, RVPT.read_frame(out=)).  Everything here is byte-exact: the comparison is always the bytes of the device read against the bytes of Context.read
(the host read) on the same context state."""
import ctypes

import numpy as np
import pytest

from _util import identity_camera, scene_by_name

pytestmark = pytest.mark.gpu

SIZES = [(96, 64), (50, 37), (16, 16)]  # 50 x 37: edge tiles in both directions, no multiple of the un-tiling block's 64 columns x 4 rows
SENTINEL = -123.25


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    n.load()
    assert n.device_count() >= 1
    return n


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def default():
    return scene_by_name("default")


def make_context(native, sc, W, H, traversal="brute", extra=0, tile_rank=0, tile_world=1):
    tris, mats, nodes = sc
    bvh = traversal == "bvh"
    ctx = native.Context(W, H, 0, tile_rank, tile_world, extra | (native.TRAVERSAL_BVH if bvh else native.TRAVERSAL_BRUTE))
    ctx.upload_scene(nodes if bvh else None, tris, mats)
    return ctx


def dispatch(ctx, W, H, frame=0, n=1, aa=2):
    from rvpt_amd import RenderSettings
    ctx.set_frame(RenderSettings(aa=aa, current_frame=frame).pack(), identity_camera(W / H))
    if n == 1:
        ctx.dispatch()
    else:
        ctx.dispatch_frames(n)


def empty_frame(torch, native, W, H, fmt, fill=None):
    dt = torch.float32 if fmt == native.FORMAT_RGBA32F else torch.uint8
    t = torch.empty((H, W, 4), dtype=dt, device="cuda:0")
    if fill is not None:
        t.fill_(fill)
    return t


def same_bytes(tensor, array):
    got = tensor.cpu().numpy()
    return got.dtype == array.dtype and got.shape == array.shape and got.tobytes() == array.tobytes()


@pytest.mark.parametrize("traversal", ["brute", "bvh"])
@pytest.mark.parametrize("fmt_name", ["RGBA32F", "RGBA8_UNORM"])
@pytest.mark.parametrize("W,H", SIZES)
def test_device_read_equals_host_read_after_a_dispatch(native, torch, default, W, H, fmt_name, traversal):
    fmt = getattr(native, "FORMAT_" + fmt_name)
    ctx = make_context(native, default, W, H, traversal)
    try:
        dispatch(ctx, W, H)
        dst = empty_frame(torch, native, W, H, fmt, fill=7)
        assert ctx.read_into(dst, fmt) is dst
        want = ctx.read(fmt)
        assert want.any()  # (a frame of the default scene, not an empty accumulator)
        assert same_bytes(dst, want)
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt_name", ["RGBA32F", "RGBA8_UNORM"])
def test_device_read_waits_for_a_chain_in_flight(native, torch, default, fmt_name):
    """dispatch_frames(6) is still in flight when the read is issued: the call implies the wait"""
    fmt = getattr(native, "FORMAT_" + fmt_name)
    W, H = 50, 37
    ctx = make_context(native, default, W, H, "bvh")
    try:
        dst = empty_frame(torch, native, W, H, fmt, fill=0)
        dispatch(ctx, W, H, frame=0, n=6)
        ctx.read_into(dst, fmt)
        got = dst.cpu().numpy()  # (taken before anything else touches the context)
        ctx.wait()
        assert got.tobytes() == ctx.read(fmt).tobytes()
        prev = None  # ... and it is the six-frame picture, not an earlier state of the accumulator: six single launches on a fresh context give it too
        fresh = make_context(native, default, W, H, "bvh")
        try:
            for f in range(6):
                dispatch(fresh, W, H, frame=f)
            prev = fresh.read(fmt)
        finally:
            fresh.close()
        assert got.tobytes() == prev.tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt_name", ["RGBA32F", "RGBA8_UNORM"])
def test_device_read_of_a_unorm8_accumulator(native, torch, default, fmt_name):
    fmt = getattr(native, "FORMAT_" + fmt_name)
    W, H = 50, 37
    ctx = make_context(native, default, W, H, "brute", extra=native.ACCUM_UNORM8)
    try:
        for f in range(3):
            dispatch(ctx, W, H, frame=f)
        dst = empty_frame(torch, native, W, H, fmt)
        ctx.read_into(dst, fmt)
        assert same_bytes(dst, ctx.read(fmt))
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt_name", ["RGBA32F", "RGBA8_UNORM"])
def test_partitioned_image_without_a_communicator(native, torch, default, fmt_name):
    """tile_world=3, tile_rank=1: the pixels of tiles the rank does not own read as 0, as on the host path"""
    from rvpt_amd.distributed import tile_grid
    fmt = getattr(native, "FORMAT_" + fmt_name)
    W, H = 96, 64
    ctx = make_context(native, default, W, H, "brute", tile_rank=1, tile_world=3)
    try:
        dispatch(ctx, W, H)
        dst = empty_frame(torch, native, W, H, fmt, fill=9)
        ctx.read_into(dst, fmt)
        want = ctx.read(fmt)
        assert same_bytes(dst, want)
        tx, ty = tile_grid(W, H)
        got = dst.cpu().numpy()
        owned = 0
        for row in range(ty):
            for col in range(tx):
                slot = row * tx + (col + native.TILE_SHIFT * row) % tx
                block = got[row * 16:(row + 1) * 16, col * 16:(col + 1) * 16]
                if slot % 3 != 1:
                    assert not block.any()
                else:
                    owned += int(block.any())
        assert owned > 0
    finally:
        ctx.close()


def test_single_rank_communicator(native, torch, default):
    """the collective read (world-1 RCCL group): gather on rank 0, then into the tensor on the device — aligned and one float into a larger tensor"""
    W, H = 50, 37
    ctx = make_context(native, default, W, H, "brute")
    try:
        dispatch(ctx, W, H)
        want, want8 = ctx.read(), ctx.read(native.FORMAT_RGBA8_UNORM)
        ctx.comm_init(native.comm_unique_id())
        assert np.array_equal(ctx.read(), want)
        dst = empty_frame(torch, native, W, H, native.FORMAT_RGBA32F, fill=3)
        ctx.read_into(dst)
        assert same_bytes(dst, want)
        dst8 = empty_frame(torch, native, W, H, native.FORMAT_RGBA8_UNORM, fill=3)
        ctx.read_into(dst8, native.FORMAT_RGBA8_UNORM)
        assert same_bytes(dst8, want8)
        big = torch.full((H * W * 4 + 8,), SENTINEL, dtype=torch.float32, device="cuda:0")
        ctx.read_into(big[1:1 + H * W * 4].view(H, W, 4))
        got = big.cpu().numpy()
        assert got[1:1 + H * W * 4].tobytes() == want.tobytes() and got[0] == SENTINEL and (got[1 + H * W * 4:] == SENTINEL).all()
        # rank 0's own bad argument: reported after the exchange, the tensor untouched
        rc = native.load().rvpt_hip_read(ctx._h, native.FORMAT_RGBA32F, ctypes.c_void_p(dst.data_ptr()), H * W * 16 - 1)
        assert rc == native.ERR_SIZE and same_bytes(dst, want)
    finally:
        ctx.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_misaligned_destination(native, torch, default, W, H):
    """a view starting one float into a larger tensor: filled correctly, the float before it and the floats after the frame keep their value"""
    ctx = make_context(native, default, W, H, "bvh")
    try:
        dispatch(ctx, W, H)
        n = H * W * 4
        big = torch.full((n + 9,), SENTINEL, dtype=torch.float32, device="cuda:0")
        view = big[1:1 + n].view(H, W, 4)
        assert view.data_ptr() % 16 == 4
        ctx.read_into(view)
        got = big.cpu().numpy()
        assert got[1:1 + n].tobytes() == ctx.read().tobytes()
        assert got[0] == SENTINEL and (got[1 + n:] == SENTINEL).all()
        # rgba8 into a view one WORD into a larger tensor
        big8 = torch.full((n + 36,), 0x5A, dtype=torch.uint8, device="cuda:0")
        view8 = big8[4:4 + n].view(H, W, 4)
        ctx.read_into(view8, native.FORMAT_RGBA8_UNORM)
        got8 = big8.cpu().numpy()
        assert got8[4:4 + n].tobytes() == ctx.read(native.FORMAT_RGBA8_UNORM).tobytes()
        assert (got8[:4] == 0x5A).all() and (got8[4 + n:] == 0x5A).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("traversal,tile", [("brute", (0, 1)), ("bvh", (0, 1)), ("brute", (1, 3))])
@pytest.mark.parametrize("W,H", [(50, 37), (96, 64)])
def test_restore_round_trip(native, torch, default, W, H, traversal, tile):
    """write_accum(tensor) == write_accum(numpy), aligned and one float into a larger tensor; continuing the accumulation for two frames gives identical frames"""
    rng = np.random.RandomState(5)
    img = rng.rand(H, W, 4).astype(np.float32)
    frames = {}
    for source in ("numpy", "tensor", "misaligned"):
        ctx = make_context(native, default, W, H, traversal, tile_rank=tile[0], tile_world=tile[1])
        try:
            dispatch(ctx, W, H, frame=0)  # (something to overwrite)
            if source == "numpy":
                ctx.write_accum(img)
            elif source == "tensor":
                ctx.write_accum(torch.from_numpy(img).to("cuda:0"))
            else:
                big = torch.zeros(H * W * 4 + 4, dtype=torch.float32, device="cuda:0")
                view = big[1:1 + H * W * 4].view(H, W, 4)
                view.copy_(torch.from_numpy(img))
                assert view.data_ptr() % 16 == 4
                ctx.write_accum(view)
            restored = ctx.read()
            for f in (1, 2):
                dispatch(ctx, W, H, frame=f)
            frames[source] = (restored, ctx.read())
        finally:
            ctx.close()
    if tile[1] == 1:
        assert frames["numpy"][0].tobytes() == img.tobytes()
    for source in ("tensor", "misaligned"):
        assert frames[source][0].tobytes() == frames["numpy"][0].tobytes()
        assert frames[source][1].tobytes() == frames["numpy"][1].tobytes()
    assert frames["numpy"][1].tobytes() != frames["numpy"][0].tobytes()  # (the two frames did accumulate)


def test_a_short_destination_is_err_size_and_stays_untouched(native, torch, default):
    W, H = 50, 37
    ctx = make_context(native, default, W, H, "brute")
    try:
        dispatch(ctx, W, H)
        L = native.load()
        for fmt, size in ((native.FORMAT_RGBA32F, 16), (native.FORMAT_RGBA8_UNORM, 4)):
            dst = empty_frame(torch, native, W, H, fmt, fill=5)
            before = dst.cpu().numpy().copy()
            rc = L.rvpt_hip_read(ctx._h, fmt, ctypes.c_void_p(dst.data_ptr()), H * W * size - 1)  # the C call, one byte short
            assert rc == native.ERR_SIZE and b"frame needs" in L.rvpt_hip_last_error(ctx._h)
            torch.cuda.synchronize()
            assert same_bytes(dst, before)
        short = torch.full((H * W * 4 - 1,), 5, dtype=torch.uint8, device="cuda:0")  # the same through the wrapper
        with pytest.raises(native.NativeError) as e:
            ctx.read_into(short, native.FORMAT_RGBA8_UNORM)
        assert e.value.code == native.ERR_SIZE and (short.cpu().numpy() == 5).all()
        src = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        want = ctx.read()
        rc = L.rvpt_hip_write_accum(ctx._h, ctypes.c_void_p(src.data_ptr()), H * W * 16 - 1)
        assert rc == native.ERR_SIZE and ctx.read().tobytes() == want.tobytes()
    finally:
        ctx.close()


def test_wrong_dtype_or_shape_is_refused_in_python(native, torch, default):
    W, H = 50, 37
    ctx = make_context(native, default, W, H, "brute")
    try:
        dispatch(ctx, W, H)
        bad = [
            (torch.zeros((H, W, 4), dtype=torch.float64, device="cuda:0"), native.FORMAT_RGBA32F),
            (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"), native.FORMAT_RGBA8_UNORM),
            (torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0"), native.FORMAT_RGBA32F),
            (torch.zeros((W, H, 4), dtype=torch.float32, device="cuda:0"), native.FORMAT_RGBA32F),
            (torch.zeros((H * W * 4,), dtype=torch.float32, device="cuda:0"), native.FORMAT_RGBA32F),
            (torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")[:, :, ::2], native.FORMAT_RGBA32F),  # right shape, not contiguous
            (np.zeros((H, W, 4), dtype=np.float64), native.FORMAT_RGBA32F),
            (np.zeros((H, W, 3), dtype=np.float32), native.FORMAT_RGBA32F),
            ([0.0] * 4, native.FORMAT_RGBA32F),
        ]
        for dst, fmt in bad:
            with pytest.raises(native.NativeError) as e:
                ctx.read_into(dst, fmt)
            assert e.value.code in (native.ERR_INVALID, native.ERR_SIZE)
            assert "read_into" in str(e.value)  # refused by the wrapper, before the call
        with pytest.raises(native.NativeError, match="write_accum"):
            ctx.write_accum(torch.zeros((H, W, 4), dtype=torch.float64, device="cuda:0"))
        with pytest.raises(native.NativeError, match="write_accum"):
            ctx.write_accum(torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda:0"))
        host = np.full((H, W, 4), 2.0, dtype=np.float32)  # a numpy destination is the host read
        assert ctx.read_into(host) is host and host.tobytes() == ctx.read().tobytes()
    finally:
        ctx.close()


def test_a_tensor_on_another_gpu_is_err_invalid(native, torch, default):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    W, H = 50, 37
    ctx = make_context(native, default, W, H, "brute")
    try:
        dispatch(ctx, W, H)
        L = native.load()
        other = torch.full((H, W, 4), 5.0, dtype=torch.float32, device="cuda:1")
        torch.cuda.synchronize(1)
        rc = L.rvpt_hip_read(ctx._h, native.FORMAT_RGBA32F, ctypes.c_void_p(other.data_ptr()), H * W * 16)
        msg = L.rvpt_hip_last_error(ctx._h)
        assert rc == native.ERR_INVALID and b"GPU 1" in msg and b"GPU 0" in msg
        assert (other.cpu().numpy() == 5.0).all()
        rc = L.rvpt_hip_write_accum(ctx._h, ctypes.c_void_p(other.data_ptr()), H * W * 16)
        msg = L.rvpt_hip_last_error(ctx._h)
        assert rc == native.ERR_INVALID and b"GPU 1" in msg and b"GPU 0" in msg
        with pytest.raises(native.NativeError, match="lives on device 1"):
            ctx.read_into(other)
    finally:
        ctx.close()


@pytest.mark.parametrize("traversal", ["brute", "bvh"])
def test_read_frame_out(native, torch, traversal):
    """RVPT.read_frame(out=t) returns t, equal to read_frame(); without out= it is what it was"""
    from rvpt_amd import RVPT, scene
    W, H = 50, 37
    tris, mats = scene.default_scene()
    r = RVPT(W, H, device=0, traversal=traversal)
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.render_settings.aa = 2
        r.initialize()
        for _ in range(2):
            r.update()
            r.draw()
        t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        assert r.read_frame(out=t) is t
        want = r.read_frame()
        assert isinstance(want, np.ndarray) and same_bytes(t, want)
        t8 = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
        assert r.read_frame(native.FORMAT_RGBA8_UNORM, out=t8) is t8
        assert same_bytes(t8, r.read_frame(native.FORMAT_RGBA8_UNORM))
    finally:
        r.shutdown()


def test_distributed_read_frame_out(native, torch, monkeypatch):
    """DistributedRVPT.read_frame(out=) on rank 0 (one rank, the library's communicator forced): the frame stays in the tensor"""
    from rvpt_amd import scene
    from rvpt_amd.distributed import DistributedRVPT
    monkeypatch.setenv("RVPT_FORCE_COLLECTIVE", "1")
    W, H = 50, 37
    tris, mats = scene.default_scene()
    d = DistributedRVPT(W, H, traversal="brute", rank=0, world=1, device=0)
    try:
        d.add_triangles(tris)
        for m in mats:
            d.add_material(m)
        assert d.initialize() and d.library_comm
        d.update()
        d.draw()
        want = d.read_frame()
        big = torch.full((H * W * 4 + 4,), SENTINEL, dtype=torch.float32, device="cuda:0")
        for t in (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0"), big[1:1 + H * W * 4].view(H, W, 4)):
            assert d.read_frame(out=t) is t
            assert same_bytes(t, want)
        assert float(big[0]) == SENTINEL
    finally:
        d.shutdown()
