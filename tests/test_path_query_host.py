"""Path queries without a GPU: the record of include/rvpt_hip.h is the record of rvpt_amd/native.py, the wrappers refuse what they can see to be wrong before
any call into the library, the numpy wang_hash is the oracle's, and the records tests/_path_query.py derives for a frame's pixels are that frame's camera rays —
shown on the pixels whose ray misses: the miss radiance of the derived direction is the rendered pixel, bit for bit."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _path_query as pq
from _util import scene_by_name

ROOT = Path(__file__).resolve().parent.parent
OFFSETS = {"org": 0, "seed": 12, "dir": 16, "max_bounces": 28, "radiance": 32, "segments": 44}


def test_the_header_record_compiles_as_c99_with_the_pinned_layout(tmp_path):
    fields = ", ".join(f"offsetof(rvpt_ray_path, {f})" for f in OFFSETS)
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu ' + " ".join(["%zu"] * len(OFFSETS)) + ' %d %u\\n", sizeof(rvpt_ray_path), '
           + fields + ", RVPT_HIP_FORMAT_RAY_PATHS, RVPT_HIP_PATH_MAX_BOUNCES);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [48, *OFFSETS.values(), 3, 1024]


def test_the_bindings_record_is_the_headers():
    from rvpt_amd import native
    assert native.RAY_PATH_DTYPE.itemsize == 48
    assert {n: native.RAY_PATH_DTYPE.fields[n][1] for n in native.RAY_PATH_DTYPE.names} == OFFSETS
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RVPT_HIP_[A-Z0-9_]+) (0x[0-9A-Fa-f]+|\d+)u?\b", text)}
    assert defs["RVPT_HIP_FORMAT_RAY_PATHS"] == native.FORMAT_RAY_PATHS == 3
    assert defs["RVPT_HIP_PATH_MAX_BOUNCES"] == native.PATH_MAX_BOUNCES == 1024
    assert defs["RVPT_HIP_ABI_VERSION"] == 8 and "Still 8, no\n" in text and "new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_RAY_PATHS" in text
    kernel_side = (ROOT / "rvpt_amd" / "csrc" / "rvpt_paths.h").read_text()
    assert int(re.search(r"constexpr uint32_t kPathMaxBounces = (\d+);", kernel_side).group(1)) == 1024


def _context_without_a_library():
    """a Context whose library handle is None: a wrapper that got as far as the call would fail with AttributeError, not with NativeError"""
    from rvpt_amd import native
    ctx = object.__new__(native.Context)
    ctx._L = ctx._h = None
    ctx.device = 0
    return ctx


def test_the_wrappers_refuse_before_any_call():
    import torch
    from rvpt_amd import native
    ctx = _context_without_a_library()
    good = np.zeros(4, dtype=native.RAY_PATH_DTYPE)
    with pytest.raises(AttributeError):  # (the helper's premise: a well-formed array does reach the call)
        ctx.trace_paths_into(good)
    refused = [
        np.zeros(4, dtype=native.RAY_HIT_DTYPE),  # the ray queries' record
        np.zeros((4, 12), dtype=np.float32),
        np.zeros(8, dtype=native.RAY_PATH_DTYPE)[::2],  # not contiguous
        torch.zeros((4, 12), dtype=torch.float64),
        torch.zeros((4, 11), dtype=torch.float32),
        torch.zeros((4, 24), dtype=torch.float32)[:, ::2],  # not contiguous
        [0.0] * 12,
    ]
    for records in refused:
        with pytest.raises(native.NativeError) as e:
            ctx.trace_paths_into(records)
        assert e.value.code == native.ERR_INVALID and "trace_paths_into" in str(e.value)
    read_only = good.copy()
    read_only.setflags(write=False)
    with pytest.raises(native.NativeError, match="writeable RAY_PATH_DTYPE"):
        ctx.trace_paths_into(read_only)
    # the same refusals, in the same words, as trace_rays_into
    for bad in (np.zeros((4, 12), dtype=np.float32), torch.zeros((4, 11), dtype=torch.float32), "records"):
        said = []
        for call, dtype_name in ((ctx.trace_rays_into, "RAY_HIT_DTYPE"), (ctx.trace_paths_into, "RAY_PATH_DTYPE")):
            with pytest.raises(native.NativeError) as e:
                call(bad)
            said.append(str(e.value).replace(call.__name__, "X").replace(dtype_name, "D"))
        assert said[0] == said[1]
    # trace_paths: mismatched lengths, and values a uint32 cannot hold
    org, dirv = np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32)
    with pytest.raises(native.NativeError, match="5 origins, 4 directions"):
        ctx.trace_paths(org, dirv[:4], 1, 8)
    with pytest.raises(native.NativeError, match="5 rays, seed of shape"):
        ctx.trace_paths(org, dirv, np.arange(4, dtype=np.uint32), 8)
    with pytest.raises(native.NativeError, match="5 rays, max_bounces of shape"):
        ctx.trace_paths(org, dirv, 1, np.full(6, 8))
    with pytest.raises(native.NativeError, match="max_bounces must be integers"):
        ctx.trace_paths(org, dirv, 1, 8.5)
    with pytest.raises(native.NativeError, match="seed must be integers"):
        ctx.trace_paths(org, dirv, -1, 8)
    with pytest.raises(AttributeError):  # well-formed: scalars and one value per ray reach the call
        ctx.trace_paths(org, dirv, np.arange(5, dtype=np.uint32), 8)
    # a frame's buffer is no place for records: the format is known, and refused by name
    with pytest.raises(native.NativeError, match="format 3 holds query records"):
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), native.FORMAT_RAY_PATHS, "read_into")
    with pytest.raises(native.NativeError, match="unknown format 4"):
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), 4, "read_into")


def test_numpy_wang_hash_is_the_oracles(oracle):
    from rvpt_amd.renderer import wang_hash
    values = np.concatenate([np.arange(600, dtype=np.uint32), np.random.RandomState(5).randint(0, 2 ** 32, 396, dtype=np.uint64).astype(np.uint32),
                             np.array([0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 61], dtype=np.uint32)])
    assert values.shape[0] == 1000
    got = wang_hash(values)
    assert got.dtype == np.uint32 and got.tolist() == [oracle.wang_hash(int(v)) for v in values]
    assert int(wang_hash(np.uint32(7))) == oracle.wang_hash(7) and int(wang_hash(7)) == oracle.wang_hash(7)  # (scalars too, without a warning)
    # ... and wang_hash(i) + frame is the state a pixel starts from: two draws later it is rand_stream's states[1], which the helper's records carry
    state = np.uint32(got[5] + np.uint32(3))
    for _ in range(2):
        state ^= np.uint32(state << np.uint32(13))
        state ^= state >> np.uint32(17)
        state ^= np.uint32(state << np.uint32(5))
    assert int(state) == int(oracle.rand_stream(5, 3, 2)[1][1])


@pytest.mark.parametrize("scene", ["default", "showcase"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sky_pixels_are_the_miss_radiance_of_the_derived_ray(oracle, scene, mode):
    """24 x 16, brute-force traversal, frame 0: for every pixel whose derived ray hits nothing (oracle.closest_hit), the miss radiance of the derived direction
    equals the rendered pixel bit for bit — the derivation of (cx, cy), of the ray and of the pixel order is the frame's."""
    from rvpt_amd.camera import Camera
    W, H = 24, 16
    tris, mats, _ = scene_by_name(scene)
    camera = Camera(W / H)
    camera.translation = np.array([0.0, 0.9, -2.5])
    cam = camera.get_data()
    img, _ = oracle.render(oracle.settings_bytes(max_bounces=8, aa=1, current_frame=0, camera_mode=mode), cam, None, tris, mats, W, H, 1)
    rec = pq.frame_records(oracle, mode, cam, W, H, 0, 8)
    assert (rec["max_bounces"] == 8).all() and (rec["segments"] == 0xCDCDCDCD).all()
    sky = np.array([oracle.closest_hit(None, tris, 1, r["org"], r["dir"])[0] < 0 for r in rec])
    assert sky.sum() >= W * H // 4, sky.sum()
    want = pq.expected_image(pq.miss_radiance(rec["dir"]), 0, W, H).reshape(-1, 3)[sky]
    got = img[..., :3].reshape(-1, 3)[sky]
    assert pq.same_bits(got, want), pq.first_difference(got, want)
    if mode == 1:  # the orthographic camera: origins vary, and the direction is a matrix column, not a unit vector made here
        assert np.unique(rec["org"], axis=0).shape[0] == W * H and np.unique(rec["dir"], axis=0).shape[0] == 1
    else:
        assert np.unique(rec["org"], axis=0).shape[0] == 1
