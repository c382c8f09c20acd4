"""The bind and the skin update without a GPU: the records of include/rvpt_hip.h are the records of rvpt_amd/native.py, scene.skin_triangles is the arithmetic the
header states (per influence the pose update's three products and three sums, then four products and three sums over the influences, each rounded to float32 on
its own: bit for bit, no tolerance anywhere), one-hot weights give the pose update's bytes, the .w lanes and the material rows are kept, and the refusals and the
reordering of the wrappers that need no device."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _skin
from test_pose_host import _fusing_would_differ, about, bits, rotation

ROOT = Path(__file__).resolve().parent.parent
SKIN_OFFSETS = {"bone": 0, "weight": 16}


def scenes():
    from rvpt_amd import scene
    out = {"default": scene.default_scene()[0], "cornell2": scene.cornell_scene(2)[0]}
    assert out["default"].shape[0] == 143 and out["cornell2"].shape[0] == 2300
    return out


def test_the_header_records_compile_as_c99_with_the_pinned_layout(tmp_path):
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu %zu %zu %zu %u %d %d\\n", sizeof(rvpt_vertex_skin), '
           "offsetof(rvpt_vertex_skin, bone), offsetof(rvpt_vertex_skin, weight), sizeof(rvpt_bone), offsetof(rvpt_bone, m), RVPT_HIP_SKIN_MAX_BONES, "
           "RVPT_HIP_NODES_BIND_SKIN == (size_t)-6 && RVPT_HIP_NODES_BIND_SKIN == RVPT_HIP_NODES_UPDATE_POSE - 1, "
           "RVPT_HIP_NODES_UPDATE_SKIN == (size_t)-7);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [32, 0, 16, 48, 0, 1024, 1, 1]


def test_the_bindings_records_are_the_headers():
    import ctypes
    from rvpt_amd import native, scene
    assert native.VERTEX_SKIN_DTYPE.itemsize == 32 and native.VERTEX_SKIN_DTYPE == scene.VERTEX_SKIN_DTYPE
    assert {n: native.VERTEX_SKIN_DTYPE.fields[n][1] for n in native.VERTEX_SKIN_DTYPE.names} == SKIN_OFFSETS
    assert native.VERTEX_SKIN_DTYPE["bone"].shape == (4,) and native.VERTEX_SKIN_DTYPE["weight"].shape == (4,)
    assert native.VERTEX_SKIN_DTYPE["bone"].base == np.dtype("<u4") and native.VERTEX_SKIN_DTYPE["weight"].base == np.dtype("<f4")
    assert native.BONE_DTYPE.itemsize == 48 and native.BONE_DTYPE["m"].shape == (12,)
    assert native.NODES_BIND_SKIN == ctypes.c_size_t(-6).value and native.NODES_UPDATE_SKIN == ctypes.c_size_t(-7).value
    assert native.SKIN_MAX_BONES == scene.SKIN_MAX_BONES == 1024
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    assert re.search(r"#define RVPT_HIP_NODES_BIND_SKIN \(\(size_t\)-6\)", text) and re.search(r"#define RVPT_HIP_NODES_UPDATE_SKIN \(\(size_t\)-7\)", text)
    assert "#define RVPT_HIP_ABI_VERSION 8" in text and "#define RVPT_HIP_SKIN_MAX_BONES 1024u" in text
    assert "the count RVPT_HIP_NODES_BIND_SKIN with `nodes` pointing at three rvpt_vertex_skin records" in text
    assert "the count RVPT_HIP_NODES_UPDATE_SKIN with `nodes` pointing at a list of rvpt_bone" in text
    assert "NO GUARDED SKIN UPDATE" in text
    lab = (ROOT / "include" / "rvpt_hip_lab.h").read_text()
    assert "RVPT_HIP_STATE_SKIN = 12" in lab and "RVPT_HIP_STATE_BONES = 13" in lab
    assert native.SCENE_STATE_PIECES["skin"] == (12, native.VERTEX_SKIN_DTYPE, ()) and native.SCENE_STATE_PIECES["bones"] == (13, np.float32, (12,))


def one_triangle(v0, v1, v2):
    tri = np.zeros((1, 16), dtype=np.float32)
    tri[0, 0:3], tri[0, 4:7], tri[0, 8:11] = v0, v1, v2
    tri[0, [3, 7, 11]], tri[0, 12] = (0.25, 0.5, 0.75), 2.0
    return tri


def test_the_arithmetic_is_unfused_float32():
    """Both stages.  The blend: weights (a, b, 0, 0) on two bones whose matrices are the constants x and y give round(round(a x) + round(b y)), where the fused
    form differs in the last bit.  The pose inside an influence: weight 1 on the matrix of the pose test, the other three influences of weight 0."""
    from rvpt_amd import scene
    a, x, b, y, unfused, fused = _fusing_would_differ()
    assert abs(int(bits(unfused)[0]) - int(bits(fused)[0])) == 1
    const = np.zeros((2, 3, 4), dtype=np.float32)
    const[0, :, 3], const[1, :, 3] = x, y  # q0 = (x, x, x), q1 = (y, y, y) whatever the vertex
    rec = np.zeros(3, dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"][:] = (0, 1, 0, 1)
    rec["weight"][:] = (a, b, 0, 0)
    tri = one_triangle((1, 2, 3), (4, 5, 6), (7, 8, 9))
    out = scene.skin_triangles(tri, rec, const)
    assert out.dtype == np.float32 and out.shape == (1, 16)
    got = out.reshape(4, 4)[:3, :3]
    assert (bits(got) == bits(unfused)).all() and (bits(got) != bits(fused)).all()
    # the inner stage: ((a x + b y) + 0 z) + 0 per row, as in the pose update's test
    m = np.array([[a, b, 0, 0], [0, a, b, 0], [b, 0, a, 0]], dtype=np.float32)
    tri = one_triangle((x, y, 0), (0, x, y), (y, 0, x))
    rec["bone"][:] = (0, 0, 0, 0)
    rec["weight"][:] = (1, 0, 0, 0)
    out = scene.skin_triangles(tri, rec, m[None]).reshape(4, 4)
    assert bits(out[0, 0]) == bits(unfused) and bits(out[1, 1]) == bits(unfused) and bits(out[2, 2]) == bits(unfused)
    assert out.reshape(16).tobytes() == scene.pose_parts(tri, [(0, 1, m)]).reshape(16).tobytes()


@pytest.mark.parametrize("name", ["default", "cornell2"])
def test_one_hot_weights_give_the_pose_updates_bytes(name):
    """two parts by range, the same two matrices as bones 0 and 1: 1 * q + 0 * q' + 0 * q' + 0 * q' is q byte for byte wherever no component is -0 (checked)"""
    from rvpt_amd import scene
    tris = scenes()[name]
    n = tris.shape[0]
    half = n // 2
    m0 = about((0, 0, 2), rotation((0.2, 1, 0.1), 0.4))
    m1 = np.array([[1.2, 0.25, 0.0, 0.05], [0.0, 0.5, 0.2, -0.1], [0.1, 0.0, 1.1, 0.2]])
    posed = scene.pose_parts(tris, [(0, half, m0), (half, n - half, m1)])
    assert _skin.no_minus_zero(posed)
    idx = np.zeros((n, 3, 4), dtype=np.int64)
    idx[half:, :, 0] = 1  # the one influence that counts
    idx[:, :, 1:] = np.array([1, 0, 1])  # the others name either bone
    w = np.zeros((n, 3, 4), dtype=np.float32)
    w[:, :, 0] = 1
    out = scene.skin_triangles(tris, (idx, w), np.stack([m0, m1]).astype(np.float32))
    assert out.tobytes() == posed.tobytes()


def test_four_equal_weights_on_one_bone_round_where_the_sum_says():
    """((0.25 q + 0.25 q) + 0.25 q) + 0.25 q against the bone's pose q.  0.25 q and 0.5 q are exact.  Write q = M 2^e with the 24-bit integer M: 0.75 q = (3 M / 4) 2^e.
    Where 3 M / 4 >= 2^23 it is rounded to an integer: M = 4 a gives 3 a, exact; M = 4 a + 1 gives 3 a + 0.75 -> 3 a + 1, and adding a + 0.25 gives 4 a + 1.25 -> M;
    M = 4 a + 3 gives 3 a + 2.25 -> 3 a + 2, plus a + 0.75 is 4 a + 2.75 -> M; M = 4 a + 2 is a tie, 3 a + 1.5: to 3 a + 2 for even a, then 4 a + 2.5 is a tie again
    and goes to the even 4 a + 2 = M; to 3 a + 1 for odd a, then 4 a + 1.5 goes to the even 4 a + 2 = M.  Where 3 M / 4 < 2^23 the grid is twice as fine, the error
    of the third step at most a quarter of q's last place, and the last sum rounds back to M.  So the rounding says: NOWHERE.  Four equal quarters are the pose,
    byte for byte, although two of the three sums round — unlike, say, three thirds."""
    from rvpt_amd import scene
    tris = scenes()["default"]
    n = tris.shape[0]
    m = about((0, 0, 2), rotation((0.3, 1, 0.2), 0.35))
    q = scene.pose_parts(tris, [(0, n, m)])
    idx = np.zeros((n, 3, 4), dtype=np.int64)
    w = np.full((n, 3, 4), 0.25, dtype=np.float32)
    out = scene.skin_triangles(tris, (idx, w), m[None])
    qv = q.reshape(-1, 4, 4)[:, :3, :3]
    quarter = np.float32(0.25) * qv
    three = (quarter + quarter) + quarter
    want = three + quarter
    assert want.dtype == np.float32
    got = out.reshape(-1, 4, 4)[:, :3, :3]
    assert (bits(got) == bits(want)).all()
    assert (three.astype(np.float64) != 0.75 * qv.astype(np.float64)).any()  # the third step does round somewhere ...
    assert out.tobytes() == q.tobytes()  # ... and the fourth undoes it everywhere
    # three thirds do not: round(1/3) three times over, the fourth influence at weight 0
    w3 = np.zeros((n, 3, 4), dtype=np.float32)
    w3[:, :, :3] = np.float32(1.0 / 3.0)
    thirds = scene.skin_triangles(tris, (idx, w3), m[None]).reshape(-1, 4, 4)[:, :3, :3]
    third = np.float32(1.0 / 3.0) * qv
    assert (bits(thirds) == bits(((third + third) + third) + np.float32(0) * qv)).all()
    ulps = np.abs(bits(thirds).astype(np.int64) - bits(qv).astype(np.int64))
    assert 0 < ulps.max() <= 2 and (ulps == 0).any()


def test_w_lanes_and_material_rows_are_kept():
    from rvpt_amd import scene
    tris = scenes()["default"].copy()
    n = tris.shape[0]
    tris[:, [3, 7, 11]] = np.arange(3 * n, dtype=np.float32).reshape(n, 3) + 0.5
    tris[:, 13:16] = np.arange(3 * n, dtype=np.float32).reshape(n, 3) - 7.0
    for k in (1, 3, 7):
        out = scene.skin_triangles(tris, _skin.weights(tris, k), _skin.bones(tris, k))
        assert out[:, [3, 7, 11]].tobytes() == tris[:, [3, 7, 11]].tobytes() and out[:, 12:].tobytes() == tris[:, 12:].tobytes()
        assert not np.array_equal(out[:, :12], tris[:, :12])


@pytest.mark.parametrize("name", ["default", "cornell2"])
@pytest.mark.parametrize("k", [1, 3, 7, 1024])
def test_the_generator_makes_finite_moved_vertices_without_minus_zero(name, k):
    """what the GPU tests' byte equality of boxes rests on (tests/test_pose_update.py: no_minus_zero)"""
    from rvpt_amd import scene
    tris = scenes()[name]
    rec, m = _skin.weights(tris, k), _skin.bones(tris, k)
    assert rec.shape == (3 * tris.shape[0],) and m.shape == (k, 3, 4) and int(rec["bone"].max()) < k
    assert np.abs(rec["weight"].astype(np.float64).sum(axis=1) - 1).max() < 1e-6
    if k < 4:
        assert not rec["weight"][:, k:].any() and not rec["bone"][:, k:].any()
    out = scene.skin_triangles(tris, rec, m)
    v = out.reshape(-1, 4, 4)[:, :3, :3]
    assert np.isfinite(v).all() and _skin.no_minus_zero(out) and _skin.no_minus_zero(tris)
    assert (bits(v) != bits(tris.reshape(-1, 4, 4)[:, :3, :3])).any(axis=2).all()  # every vertex moved
    again = scene.skin_triangles(tris, rec, _skin.bones(tris, k, phase=1.0))
    assert again.tobytes() != out.tobytes()


def test_the_wrappers_refusals():
    from rvpt_amd import native, scene
    tris = scenes()["default"]
    n = tris.shape[0]
    idx, w = np.zeros((n, 3, 4), dtype=np.int64), np.zeros((n, 3, 4), dtype=np.float32)
    eye = np.tile(np.eye(3, 4, dtype=np.float32), (2, 1, 1))
    ctx = native.Context.__new__(native.Context)  # no library needed: the lists are refused before any call
    neg, big = idx.copy(), idx.copy()
    neg[3, 1, 2], big[4, 2, 0] = -1, 2 ** 32
    for args, what in (((idx[:, :2], w[:, :2]), r"\[n, 3, 4\]"), ((idx, w[:-1]), r"\[n, 3, 4\]"), ((idx.astype(np.float32), w), "integers"),
                       ((neg, w), r"skin\[10\]\.bone\[2\] = -1"), ((big, w), r"skin\[14\]\.bone\[0\] = 4294967296"),
                       ((np.zeros(7, dtype=scene.VERTEX_SKIN_DTYPE),), "not three per triangle"), ((np.zeros((n, 8), dtype=np.float32),), "VERTEX_SKIN_DTYPE")):
        with pytest.raises(ValueError, match=what):
            scene.vertex_skins(*args)
        with pytest.raises(native.NativeError, match=what) as e:
            native.Context.bind_skin(ctx, *args)
        assert e.value.code == native.ERR_INVALID
    bad_row = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    bad_row[1, 3] = (0, 0, 0, 2)
    for bones, what in ((bad_row, r"bones\[1\]: the last row"), (np.zeros((2, 3, 3), dtype=np.float32), r"\[k, 3, 4\]"), (np.zeros((1025, 12), dtype=np.float32), "at most 1024"),
                        (np.zeros(12, dtype=np.float32), r"\[k, 3, 4\]")):
        with pytest.raises(ValueError, match=what):
            scene.bone_matrices(bones)
        with pytest.raises(native.NativeError, match=what) as e:
            native.Context.skin(ctx, bones)
        assert e.value.code == native.ERR_INVALID
    assert scene.bone_matrices(np.tile(np.eye(4), (5, 1, 1))).tolist() == np.tile(np.eye(3, 4).reshape(12), (5, 1)).tolist()
    # the statement's own: shape mismatch, a bone index >= len(bones), more than 1024 bones
    rec = scene.vertex_skins(idx, w)
    assert rec.shape == (3 * n,) and scene.vertex_skins((idx, w)).tobytes() == rec.tobytes() and scene.vertex_skins(rec.reshape(n, 3)).tobytes() == rec.tobytes()
    with pytest.raises(ValueError, match=f"{3 * n} records for {n - 1} triangles"):
        scene.skin_triangles(tris[:-1], rec, eye)
    two = idx.copy()
    two[5, 0, 3], two[9, 1, 1] = 2, 7
    with pytest.raises(ValueError, match=r"skin\[15\]\.bone\[3\] = 2 with 2 bones"):
        scene.skin_triangles(tris, (two, w), eye)
    with pytest.raises(ValueError, match="at most 1024"):
        scene.skin_triangles(tris, rec, np.zeros((1025, 3, 4), dtype=np.float32))


def test_the_mirror_reorders_the_records_into_leaf_order():
    """RVPT.bind_skin after a host build (no device: the context is a recorder): the records of the triangles as ADDED go down in leaf order, three per triangle
    kept together; RVPT.skin sends the matrices as given and keeps the host copies and bvh_nodes on scene.skin_triangles; two skin updates do not compose."""
    from rvpt_amd import RVPT, native, scene
    tris, mats = scene.default_scene()
    nodes, order = native.build_bvh(tris)
    order = np.asarray(order).astype(np.int64)

    class Recorder:
        def __init__(self):
            self.bound, self.bones = [], []

        def bind_skin(self, rec):
            self.bound.append(np.array(rec, copy=True))

        def skin(self, m):
            self.bones.append(np.array(m, copy=True))

        def pose_parts(self, rec):
            pass

    r = RVPT(64, 48, traversal="bvh")
    r.add_triangles(tris)
    r._n_triangles, r._ctx = tris.shape[0], Recorder()
    r.bvh_nodes, r.primitive_indices, r.sorted_triangles = nodes, order, tris[order]
    rec, m = _skin.weights(tris, 7), _skin.bones(tris, 7)
    with pytest.raises(native.NativeError, match="before a bind"):
        r.skin(m)
    assert r.bind_skin(rec) is None
    (sent,) = r._ctx.bound
    assert sent.dtype == native.VERTEX_SKIN_DTYPE and sent.shape == (3 * tris.shape[0],)
    assert sent.tobytes() == rec.reshape(-1, 3)[order].tobytes() and sent.tobytes() != rec.tobytes()
    # ... which is the binding of the sorted triangles: skinning the leaf order with it is the leaf order of skinning the added order
    skinned = scene.skin_triangles(tris, rec, m)
    assert scene.skin_triangles(tris[order], sent, m).tobytes() == skinned[order].tobytes()
    assert r.skin(m) is None
    assert len(r._ctx.bones) == 1 and r._ctx.bones[0].tobytes() == m.reshape(-1, 12).tobytes()
    assert np.concatenate(r.triangles).tobytes() == skinned.tobytes() and r.sorted_triangles.tobytes() == skinned[order].tobytes()
    assert r.bvh_nodes.tobytes() == scene.refit_bvh(nodes, skinned[order]).tobytes()
    m2 = _skin.bones(tris, 7, phase=2.0)
    r.skin(m2)
    assert np.concatenate(r.triangles).tobytes() == scene.skin_triangles(tris, rec, m2).tobytes()
    # a pose of one part after a skin update: from the rest pose, the others stay skinned
    move = [(10, 40, about((0, 0, 2), rotation((0, 1, 0), 0.3)))]
    r.pose_parts(move)
    assert np.concatenate(r.triangles).tobytes() == scene.pose_parts(tris, move, current=scene.skin_triangles(tris, rec, m2)).tobytes()
    for bad, what in ((rec[:-3], "three per triangle"), ((np.zeros((143, 3, 4)), np.zeros((143, 3, 4))), "integers")):
        with pytest.raises(native.NativeError, match=what):
            r.bind_skin(bad)
    with pytest.raises(native.NativeError, match=r"bone\[\d\] = \d with 3 bones"):
        r.skin(m[:3])
    assert len(r._ctx.bound) == 1 and len(r._ctx.bones) == 2
