"""The geometry read-back without a GPU: the record and the two formats of include/rvpt_hip.h are those of rvpt_amd/native.py; the numpy statement
(rvpt_amd/scene.py: surface_points, triangle_unit_normals) computes what the header specifies — the point unfused, the normal the ORACLE's, bit for bit; the
invalid-record rule; the wrappers refuse what they can see to be wrong before any call, in trace_rays_into's words."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _path_query as pq
import _ray_query as rq
from _util import identity_camera

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rvpt_hip.h"
OFFSETS = {"prim": 0, "u": 4, "v": 8, "flags": 12, "point": 16, "mat": 28, "normal": 32, "reserved": 44}
F = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_the_header_record_compiles_as_c99_with_the_pinned_layout(tmp_path):
    fields = ", ".join(f"offsetof(rvpt_surface_point, {f})" for f in OFFSETS)
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu ' + " ".join(["%zu"] * len(OFFSETS)) + ' %d %d %zu\\n", '
           "sizeof(rvpt_surface_point), " + fields + ", RVPT_HIP_FORMAT_TRIANGLES, RVPT_HIP_FORMAT_SURFACE_POINTS, sizeof(rvpt_triangle));return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [48, *OFFSETS.values(), 5, 6, 64]


def test_the_bindings_record_is_the_headers():
    from rvpt_amd import native, scene
    assert native.SURFACE_POINT_DTYPE.itemsize == 48 and scene.SURFACE_POINT_DTYPE == native.SURFACE_POINT_DTYPE
    assert {n: native.SURFACE_POINT_DTYPE.fields[n][1] for n in native.SURFACE_POINT_DTYPE.names} == OFFSETS
    # the last float4 of an rvpt_point_hit is a valid in-quad
    assert [native.POINT_HIT_DTYPE.fields[n][1] - 32 for n in ("prim", "u", "v")] == [OFFSETS[n] for n in ("prim", "u", "v")]
    text = HEADER.read_text()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RVPT_HIP_[A-Z0-9_]+) (0x[0-9A-Fa-f]+|\d+)u?\b", text)}
    assert defs["RVPT_HIP_FORMAT_TRIANGLES"] == native.FORMAT_TRIANGLES == 5
    assert defs["RVPT_HIP_FORMAT_SURFACE_POINTS"] == native.FORMAT_SURFACE_POINTS == 6
    assert defs["RVPT_HIP_ABI_VERSION"] == native.ABI_VERSION == 8 and len(native.EXPORTS) == 30
    kernel_side = (ROOT / "rvpt_amd" / "csrc" / "rvpt_surface.h").read_text()
    assert int(re.search(r"constexpr uint32_t kSurfaceRecordBytes = (\d+);", kernel_side).group(1)) == 48


def test_the_headers_sentences():
    raw = HEADER.read_text()
    version_comment = raw[:raw.index("/* ---- POD layouts")]
    for n, name in ((5, "TRIANGLES"), (6, "SURFACE_POINTS")):
        assert re.search(rf"Still 8, no new\s+symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_{name} \({n}\) — until then the \"unknown\s+format\" error", version_comment)
    text = " ".join(raw.replace(" * ", " ").split())
    # the two pinned sentences stay where they are
    assert "Format 26 and every other value are the \"unknown format\" error." in text
    assert "NO GUARDED SKIN UPDATE" in text
    assert text.index("NEAREST POINTS — the nearest point") < text.index("TRIANGLES — the whole mesh as it now stands") < text.index("SURFACE POINTS — points on the stored mesh")
    for sentence in ("Row perm[s] of the answer is stored row s.",
                     "Nothing is recomputed; a NaN payload in a w lane comes back as it went in.",
                     "Passing the answer straight to the plain update form moves nothing.",
                     "gives the tree a guarded rebuild would give.",
                     "is RVPT_HIP_ERR_SIZE, and the message gives both numbers.",
                     "The empty scene is a successful no-op, and `dst` may then be NULL.",
                     "u weights vert1 - vert0 and v weights vert2 - vert0: what both query forms report.",
                     "point = (a + ab*u) + ac*v per component.",
                     "For a ray hit it is NOT org + t*dir",
                     "any finite pair is evaluated.",
                     "NOT turned towards any ray.",
                     "INVALID RECORDS are prim >= n_tris (so 0xFFFFFFFF, a miss piped through, is invalid) or a non-finite u or v.",
                     "mat = 0xFFFFFFFF, reserved = 0.",
                     "The last float4 of an rvpt_point_hit is already a valid in-quad."):
        assert sentence in text, sentence


@pytest.fixture(scope="module")
def default_tris():
    from rvpt_amd import scene
    tris, mats = scene.default_scene()
    assert tris.shape[0] == 143
    return tris, mats


def test_the_statement_at_the_corners_and_unfused(default_tris):
    from rvpt_amd import scene
    tris, _ = default_tris
    n = tris.shape[0]
    prim = np.arange(n, dtype=np.uint32)
    a, b, c = tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]
    at_a = scene.surface_points(tris, prim, 0.0, 0.0)
    assert at_a.dtype == scene.SURFACE_POINT_DTYPE and (at_a["reserved"] == 0).all() and (at_a["flags"] == 0).all()
    assert bits(at_a["point"]).tobytes() == bits(a).tobytes()  # (0, 0): a's bytes
    at_b = scene.surface_points(tris, prim, 1.0, 0.0)
    assert bits(at_b["point"]).tobytes() == bits(a + (b - a)).tobytes()  # (1, 0): a + (b - a), one rounding each ...
    at_c = scene.surface_points(tris, prim, 0.0, 1.0)
    assert bits(at_c["point"]).tobytes() == bits(a + (c - a)).tobytes()
    # ... which is not b: a chosen triangle whose a and b differ in magnitude
    chosen = scene.make_triangles([((1.0, 1.0, 1.0), (1e-8, 3.0, 2.0), (0.0, 0.0, 5.0))], 0)
    got = scene.surface_points(chosen, [0], 1.0, 0.0)["point"][0]
    assert got[0] == F(0.0) and chosen[0, 4] == F(1e-8) and got[1] == F(3.0)  # 1 + (1e-8 - 1) == 0 in float32
    assert (scene.surface_points(tris, prim, 1.0, 0.0)["mat"] == tris[:, 12].astype(np.uint32)).all()
    # a fused evaluation — (a + ab*u) and (.. + ac*v) each contracted, the product exact in float64 — changes bits somewhere on the default scene
    rng = np.random.RandomState(5)
    u, v = rng.uniform(0, 1, n).astype(F), rng.uniform(0, 1, n).astype(F)
    want = scene.surface_points(tris, prim, u, v)["point"]
    ab, ac = (b - a).astype(np.float64), (c - a).astype(np.float64)
    step = (a.astype(np.float64) + ab * u[:, None].astype(np.float64)).astype(F)
    fused = (step.astype(np.float64) + ac * v[:, None].astype(np.float64)).astype(F)
    unfused = (a + (b - a) * u[:, None]) + (c - a) * v[:, None]
    assert bits(want).tobytes() == bits(unfused).tobytes()
    assert (bits(fused) != bits(want)).any() and np.allclose(fused, want, rtol=1e-5, atol=1e-6)


def test_fmaf_is_fused():
    from rvpt_amd import scene
    x = F(1.0) + F(2.0 ** -23)
    assert scene._fmaf(x, x, -F(x * x))[()] == F(2.0 ** -46)  # the product's low half survives: one rounding
    assert scene._fmaf(np.array([1.0, 2.0], F), F(3.0), F(1.0)).tolist() == [4.0, 7.0]


def test_the_statements_normal_is_the_oracles(oracle, default_tris):
    """Render mode 3 of the oracle is fma(0.5, normal, 0.5 * hit) per channel: at every pixel whose camera ray hits, the pixel must be fmaf(0.5, n, 0.5) of the
    statement's normal for the triangle _ray_query.Statement finds for that pixel's ray, bit for bit."""
    from rvpt_amd import scene
    tris, mats = default_tris
    W, H = 64, 36
    v = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    cam = identity_camera(W / H)
    cam[12:15] = (lo + hi) / 2 - np.array([0.0, 0.0, 0.5 * float((hi - lo).max())])  # half an extent in front of the model: a third of the pixels hit
    img, _ = oracle.render(oracle.settings_bytes(max_bounces=8, aa=1, current_frame=0, modes=(3, 3, 3, 3)), cam, None, tris, mats, W, H, 1)
    rec = pq.frame_records(oracle, 0, cam, W, H, 0, 8)
    rays = rq.make_records(rec["org"], rec["dir"])
    hits = rq.Statement(oracle, None, tris).answer(rays, 1)
    hit = hits["prim"] != rq.NO_PRIM
    assert hit.sum() > W * H // 4, hit.sum()
    surf = scene.surface_points(tris, hits["prim"], hits["u"], hits["v"])
    assert ((surf["mat"] == scene.NO_PRIM) == ~hit).all()
    want = scene._fmaf(F(0.5), surf["normal"][hit], F(0.5))
    got = img[..., :3].reshape(-1, 3)[hit]
    assert pq.same_bits(got, want), pq.first_difference(got, want)
    assert len(np.unique(hits["prim"][hit])) > 20  # (many triangles, hence many normals)
    lengths = np.linalg.norm(surf["normal"][hit].astype(np.float64), axis=1)
    assert np.abs(lengths - 1).max() < 1e-6


def test_invalid_records(default_tris):
    from rvpt_amd import scene
    tris, _ = default_tris
    n = tris.shape[0]
    prim = np.array([0, n - 1, n, 0xFFFFFFFF, 3, 4, 5, 6], dtype=np.uint32)
    u = np.array([0.25, 0.25, 0.25, 0.25, np.nan, 0.25, np.inf, -3.5], dtype=F)
    v = np.array([0.5, 0.5, 0.5, 0.5, 0.5, -np.inf, 0.5, 7.25], dtype=F)
    got = scene.surface_points(tris, prim, u, v)
    valid = np.array([True, True, False, False, False, False, False, True])
    assert ((got["mat"] != scene.NO_PRIM) == valid).all()
    assert (bits(got["point"][~valid]) == 0).all() and (bits(got["normal"][~valid]) == 0).all() and (got["reserved"] == 0).all()
    assert (got["prim"] == prim).all() and bits(got["u"]).tobytes() == bits(u).tobytes() and bits(got["v"]).tobytes() == bits(v).tobytes()
    assert np.isfinite(got["point"][valid]).all() and (np.abs(got["normal"][valid]).sum(axis=1) > 0).all()  # a pair outside [0, 1] is evaluated
    empty = scene.surface_points(np.zeros((0, 16), F), prim, u, v)  # on the empty scene every record is invalid
    assert (empty["mat"] == scene.NO_PRIM).all() and (bits(empty["point"]) == 0).all()
    assert scene.surface_points(tris, np.zeros(0, np.uint32), np.zeros(0, F), np.zeros(0, F)).shape == (0,)


def _context():
    from rvpt_amd import native
    ctx = object.__new__(native.Context)
    ctx._L, ctx._h = None, None
    ctx.device = 0
    ctx._scene_tris = 4
    return ctx


def test_the_wrappers_refuse_before_any_call():
    import torch
    from rvpt_amd import RVPT, native
    ctx = _context()
    good = np.zeros(4, dtype=native.SURFACE_POINT_DTYPE)
    with pytest.raises(AttributeError):  # (the helper's premise: a well-formed array does reach the call)
        ctx.surface_points_into(good)
    refused = [
        np.zeros(4, dtype=native.RAY_HIT_DTYPE),
        np.zeros((4, 12), dtype=np.float32),
        np.zeros(8, dtype=native.SURFACE_POINT_DTYPE)[::2],  # not contiguous
        torch.zeros((4, 12), dtype=torch.float64),
        torch.zeros((4, 11), dtype=torch.float32),
        torch.zeros((4, 24), dtype=torch.float32)[:, ::2],  # not contiguous
        [0.0] * 12,
    ]
    for records in refused:
        with pytest.raises(native.NativeError) as e:
            ctx.surface_points_into(records)
        assert e.value.code == native.ERR_INVALID and "surface_points_into" in str(e.value)
    read_only = good.copy()
    read_only.setflags(write=False)
    with pytest.raises(native.NativeError, match="writeable SURFACE_POINT_DTYPE"):
        ctx.surface_points_into(read_only)
    for bad in (np.zeros((4, 12), dtype=np.float32), torch.zeros((4, 11), dtype=torch.float32), "records"):  # the same refusals, in the same words, as trace_rays_into
        said = []
        for call, dtype_name in ((ctx.trace_rays_into, "RAY_HIT_DTYPE"), (ctx.surface_points_into, "SURFACE_POINT_DTYPE")):
            with pytest.raises(native.NativeError) as e:
                call(bad)
            said.append(str(e.value).replace(call.__name__, "X").replace(dtype_name, "D"))
        assert said[0] == said[1]
    with pytest.raises(native.NativeError, match=r"prim must be integers in \[0, 2\^32\)"):
        ctx.surface_points(np.zeros(3, np.float32), 0.0, 0.0)
    with pytest.raises(native.NativeError, match=r"prim must be integers in \[0, 2\^32\)"):
        ctx.surface_points(np.array([-1, 2]), 0.0, 0.0)
    with pytest.raises(native.NativeError, match="3 records, u of shape"):
        ctx.surface_points(np.zeros(3, np.uint32), np.zeros(2, F), 0.0)
    with pytest.raises(native.NativeError, match="3 records, v of shape"):
        ctx.surface_points(np.zeros(3, np.uint32), 0.0, np.zeros((3, 1), F))
    # read_triangles_into: float32[n, 16], contiguous, writeable
    with pytest.raises(AttributeError):
        ctx.read_triangles_into(np.zeros((4, 16), np.float32))
    for dst in (np.zeros((4, 12), np.float32), np.zeros((4, 16), np.float64), np.zeros((8, 16), np.float32)[::2], np.zeros(64, np.float32),
                torch.zeros((4, 16), dtype=torch.float64), torch.zeros((4, 15), dtype=torch.float32), torch.zeros((4, 32), dtype=torch.float32)[:, ::2], "rows"):
        with pytest.raises(native.NativeError) as e:
            ctx.read_triangles_into(dst)
        assert e.value.code == native.ERR_INVALID and "read_triangles_into" in str(e.value)
    read_only = np.zeros((4, 16), np.float32)
    read_only.setflags(write=False)
    with pytest.raises(native.NativeError, match=r"writeable float32\[n, 16\]"):
        ctx.read_triangles_into(read_only)
    with pytest.raises(RuntimeError, match="surface_points before initialize"):
        RVPT(8, 8).surface_points([0], [0.0], [0.0])
    with pytest.raises(RuntimeError, match="read_triangles before initialize"):
        RVPT(8, 8).read_triangles()


def test_frame_buffer_refuses_the_two_formats_in_words_of_their_own():
    from rvpt_amd import native
    ctx = _context()
    ctx.width = ctx.height = 2
    with pytest.raises(native.NativeError, match="format 5 holds the stored triangle rows, not a frame: use read_triangles") as e:
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), native.FORMAT_TRIANGLES, "read_into")
    assert e.value.code == native.ERR_INVALID
    with pytest.raises(native.NativeError, match="format 6 holds surface records, not a frame: use surface_points") as e:
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), native.FORMAT_SURFACE_POINTS, "read_into")
    assert e.value.code == native.ERR_INVALID
    with pytest.raises(native.NativeError, match="unknown format 4"):  # (pinned elsewhere: stays)
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), 4, "read_into")
    with pytest.raises(native.NativeError, match="unknown format 7"):
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), 7, "read_into")


def test_rvpt_surface_points_takes_query_records():
    """RVPT.surface_points with a RAY_HIT_DTYPE / POINT_HIT_DTYPE array takes its prim, u, v; after a host build the added numbers go down through the inverse
    of primitive_indices and come back as given — against a recording stand-in for the context"""
    from rvpt_amd import RVPT, native

    class Recorder:
        def surface_points(self, prim, u, v):
            self.seen = (np.asarray(prim).copy(), np.asarray(u).copy(), np.asarray(v).copy())
            rec = np.zeros(np.asarray(prim).size, dtype=native.SURFACE_POINT_DTYPE)
            rec["prim"] = prim
            return rec

    r = RVPT(8, 8)
    r._ctx, r._device_built, r._n_triangles = Recorder(), False, 4
    r.primitive_indices = np.array([2, 0, 3, 1], dtype=np.uint32)  # stored row s is added triangle primitive_indices[s]
    hits = np.zeros(5, dtype=native.RAY_HIT_DTYPE)
    hits["prim"], hits["u"], hits["v"] = [0, 1, 2, 3, native.NO_PRIM], [0.1, 0.2, 0.3, 0.4, 0.0], [0.5, 0.4, 0.3, 0.2, 0.0]
    out = r.surface_points(hits)
    assert r._ctx.seen[0].tolist() == [1, 3, 0, 2, native.NO_PRIM] and out["prim"].tolist() == hits["prim"].tolist()
    assert bits(r._ctx.seen[1]).tolist() == bits(hits["u"]).tolist() and bits(r._ctx.seen[2]).tolist() == bits(hits["v"]).tolist()
    pts = np.zeros(2, dtype=native.POINT_HIT_DTYPE)
    pts["prim"], pts["u"] = [3, 7], [0.25, 0.5]
    r.surface_points(pts)
    assert r._ctx.seen[0].tolist() == [2, native.NO_PRIM] and r._ctx.seen[1].tolist() == [0.25, 0.5]
    r._device_built = True
    r.surface_points(pts)
    assert r._ctx.seen[0].tolist() == [3, 7]
    with pytest.raises(native.NativeError, match="carry their own u and v"):
        r.surface_points(pts, 0.0, 0.0)
    with pytest.raises(native.NativeError, match="prim, u and v are needed"):
        r.surface_points([1, 2])
    r._ctx = None
