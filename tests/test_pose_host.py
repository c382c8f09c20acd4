"""The pose update without a GPU: the record of include/rvpt_hip.h is the record of rvpt_amd/native.py, scene.pose_parts is the arithmetic the header states
(three products and three sums per component, each rounded to float32 on its own: bit for bit, no tolerance anywhere), the statement's rules — parts not
listed keep their pose, two poses of one part do not compose, the sparse refit over the listed positions is the refit of the posed scene — and the refusals of
the wrappers that need no device."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
OFFSETS = {"m": 0, "first": 48, "count": 52, "reserved": 56}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def about(centre, rot):
    """the 3x4 matrix of x -> R (x - c) + c"""
    c = np.asarray(centre, dtype=np.float64)
    return np.concatenate([rot, (c - rot @ c).reshape(3, 1)], axis=1)


def test_the_header_record_compiles_as_c99_with_the_pinned_layout(tmp_path):
    fields = ", ".join(f"offsetof(rvpt_part_move, {f})" for f in OFFSETS)
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu ' + " ".join(["%zu"] * len(OFFSETS)) + ' %d\\n", sizeof(rvpt_part_move), '
           + fields + ", RVPT_HIP_NODES_UPDATE_POSE == (size_t)-5 && RVPT_HIP_NODES_UPDATE_POSE == RVPT_HIP_NODES_UPDATE_SPARSE - 1);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [64, *OFFSETS.values(), 1]


def test_the_bindings_record_is_the_headers():
    import ctypes
    from rvpt_amd import native, scene
    assert native.PART_MOVE_DTYPE.itemsize == 64 and native.PART_MOVE_DTYPE == scene.PART_MOVE_DTYPE
    assert {n: native.PART_MOVE_DTYPE.fields[n][1] for n in native.PART_MOVE_DTYPE.names} == OFFSETS
    assert native.PART_MOVE_DTYPE["m"].shape == (12,) and native.PART_MOVE_DTYPE["reserved"].shape == (2,)
    assert native.NODES_UPDATE_POSE == ctypes.c_size_t(-5).value == native.NODES_UPDATE_SPARSE - 1
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    assert re.search(r"#define RVPT_HIP_NODES_UPDATE_POSE \(\(size_t\)-5\)", text)
    assert "#define RVPT_HIP_ABI_VERSION 8" in text and "Still 8, no\n" in text and "the count RVPT_HIP_NODES_UPDATE_POSE with `nodes` pointing at a list of rvpt_part_move records" in text
    lab = (ROOT / "include" / "rvpt_hip_lab.h").read_text()
    assert "RVPT_HIP_STATE_REST = 11" in lab and native.SCENE_STATE_PIECES["rest"] == (11, np.float32, (12,))


def _fusing_would_differ():
    """(a, x, b, y) in float32 for which round(round(a x) + round(b y)) differs from the fused round(a x + round(b y)) in the last bit: found by search, the
    fused value taken in float64 (a product of two float32 is exact there, and so is its sum with a float32 of like size up to one rounding)"""
    rng = np.random.RandomState(5)
    a, x, b, y = (rng.uniform(0.5, 2.0, 4096).astype(np.float32) for _ in range(4))
    unfused = a * x + b * y
    assert unfused.dtype == np.float32
    fused = (a.astype(np.float64) * x.astype(np.float64) + (b * y).astype(np.float64)).astype(np.float32)
    differ = np.flatnonzero(bits(unfused) != bits(fused))
    assert differ.size > 0
    j = int(differ[0])
    return a[j], x[j], b[j], y[j], unfused[j], fused[j]


def test_the_arithmetic_is_unfused_float32():
    from rvpt_amd import scene
    a, x, b, y, unfused, fused = _fusing_would_differ()
    assert abs(int(bits(unfused)[0]) - int(bits(fused)[0])) == 1
    # row 0 = (a, b, 0, 0) on the vertex (x, y, 0): ((a x + b y) + 0 z) + 0; rows 1 and 2 put the same pair on other columns
    m = np.array([[a, b, 0, 0], [0, a, b, 0], [b, 0, a, 0]], dtype=np.float32)
    tri = np.zeros((1, 16), dtype=np.float32)
    tri[0, 0:3], tri[0, 4:7], tri[0, 8:11] = (x, y, 0), (0, x, y), (y, 0, x)
    tri[0, [3, 7, 11]], tri[0, 12] = (0.25, 0.5, 0.75), 2.0
    out = scene.pose_parts(tri, [(0, 1, m)])
    assert out.dtype == np.float32 and out.shape == (1, 16)
    assert bits(out[0, 0]) == bits(unfused) and bits(out[0, 5]) == bits(unfused) and bits(out[0, 10]) == bits(unfused)
    assert out[0, [3, 7, 11]].tolist() == [0.25, 0.5, 0.75] and out[0, 12] == 2.0  # the w lanes and the material row stay
    # the translation is a fourth, separate rounding: 1 + 2^-24 rounds back to 1 before anything else could absorb it
    big = np.float32(1.0)
    m2 = np.array([[1, 0, 0, 2.0 ** -24], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
    tri2 = np.zeros((1, 16), dtype=np.float32)
    tri2[0, 0] = big
    assert bits(scene.pose_parts(tri2, [(0, 1, m2)])[0, 0]) == bits(np.float32(1.0))
    # a hand-computed case: x = 1 + 2^-12, x * x = 1 + 2^-11 + 2^-24 rounds (to even) to 1 + 2^-11, minus 1 leaves 2^-11; fused it would be 2^-11 + 2^-24
    xx = np.float32(1 + 2.0 ** -12)
    m3 = np.array([[xx, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
    tri3 = np.zeros((1, 16), dtype=np.float32)
    tri3[0, 0] = xx
    assert scene.pose_parts(tri3, [(0, 1, m3)])[0, 0] == np.float32(2.0 ** -11)


def test_identity_turns_minus_zero_into_plus_zero():
    from rvpt_amd import scene
    tri = np.zeros((2, 16), dtype=np.float32)
    tri[:, [0, 5, 10]] = -0.0
    tri[:, [1, 2]] = (3.0, -4.0)
    assert np.signbit(tri[0, 0])
    out = scene.pose_parts(tri, [scene.part_move(0, 1)])
    assert not np.signbit(out[0, [0, 5, 10]]).any() and (out[0, [0, 5, 10]] == 0).all() and out[0, 1] == 3.0 and out[0, 2] == -4.0
    assert np.signbit(out[1, [0, 5, 10]]).all()  # the triangle not listed keeps its bytes
    assert out[1].tobytes() == tri[1].tobytes()


def test_parts_not_listed_keep_current_and_poses_do_not_compose(default_scene):
    from rvpt_amd import scene
    tris = default_scene[0]
    n = tris.shape[0]
    centre = tris[:63].reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).mean(axis=0)
    A = (0, 63, about(centre, rotation((0, 1, 0), 0.4)))
    B = (0, 63, about(centre, rotation((1, 0, 0), -0.3)))
    C = scene.part_move(64, n - 64, translation=(0.1, 0.2, -0.3))
    after_a = scene.pose_parts(tris, [A])
    assert after_a[63:].tobytes() == tris[63:].tobytes() and not np.array_equal(bits(after_a[:63]), bits(tris[:63]))
    # B of the same part: from the rest pose, A forgotten
    after_b = scene.pose_parts(tris, [B], current=after_a)
    assert after_b.tobytes() == scene.pose_parts(tris, [B]).tobytes()
    composed = scene.pose_parts(after_a, [B])  # what composing would have given
    assert composed.tobytes() != after_b.tobytes()
    # C of another part: the first part stays at A, triangle 63 where it was
    after_c = scene.pose_parts(tris, [C], current=after_a)
    assert after_c[:63].tobytes() == after_a[:63].tobytes() and after_c[63].tobytes() == tris[63].tobytes()
    assert after_c[64:].tobytes() == scene.pose_parts(tris, [C])[64:].tobytes()
    # both at once, in either order of the list, as a structured array or as tuples
    rec = scene.part_moves([A, C])
    assert rec.dtype == scene.PART_MOVE_DTYPE and rec["first"].tolist() == [0, 64] and rec["count"].tolist() == [63, n - 64] and not rec["reserved"].any()
    assert scene.pose_parts(tris, rec).tobytes() == scene.pose_parts(tris, rec[::-1].copy()).tobytes() == after_c.tobytes()
    # a 4x4 matrix with the last row 0 0 0 1 is its upper three rows
    m4 = np.concatenate([about(centre, rotation((0, 1, 0), 0.4)), [[0, 0, 0, 1]]])
    assert scene.pose_parts(tris, [(0, 63, m4)]).tobytes() == after_a.tobytes()
    # the material rows are current's, the w lanes the rest pose's
    marked = after_a.copy()
    marked[:, 12] = 1.0
    marked[:, 3] = 9.0
    out = scene.pose_parts(tris, [B], current=marked)
    assert (out[:, 12] == 1.0).all() and (out[:63, 3] == tris[:63, 3]).all() and (out[63:, 3] == 9.0).all()


@pytest.mark.parametrize("loose", [False, True])
def test_the_sparse_refit_over_the_listed_positions(default_scene, loose):
    """refit_bvh(nodes, posed, touched=listed) equals refit_bvh(nodes, posed) on every node of the touched paths and the old nodes elsewhere."""
    from rvpt_amd import native, scene
    from test_gpu_parity import _loosen_boxes
    tris, _, nodes = default_scene
    if loose:
        nodes = _loosen_boxes(nodes, 5)
    moves = [(20, 31, about((0, 0, 2), rotation((0, 0, 1), 0.5))), scene.part_move(100, 1, translation=(0.3, 0, 0))]
    listed = np.concatenate([np.arange(20, 51), [100]])
    posed = scene.pose_parts(tris, moves)
    sparse = scene.refit_bvh(nodes, posed, touched=listed).view(native.NODE_DTYPE).reshape(-1)
    full = scene.refit_bvh(nodes, posed).view(native.NODE_DTYPE).reshape(-1)
    old = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)
    # the touched paths, from the topology: every leaf whose range holds a listed position, and its ancestors
    parent = np.full(old.shape[0], -1)
    on_path = np.zeros(old.shape[0], dtype=bool)
    stack = [0]
    while stack:
        i = stack.pop()
        if old["count"][i] == 0:
            for c in (old["first"][i], old["first"][i] + 1):
                parent[c] = i
                stack.append(int(c))
        elif ((listed >= old["first"][i]) & (listed < old["first"][i] + old["count"][i])).any():
            on_path[i] = True
    for i in np.flatnonzero(on_path):
        while parent[i] >= 0 and not on_path[parent[i]]:
            i = parent[i]
            on_path[i] = True
    assert on_path[0] and 0 < on_path.sum() < old.shape[0]
    assert sparse[~on_path].tobytes() == old[~on_path].tobytes()
    assert sparse[on_path].tobytes() != old[on_path].tobytes()
    if not loose:  # the built tree is tight: on the touched paths the sparse refit is the full one
        assert sparse[on_path].tobytes() == full[on_path].tobytes()
        return
    # a caller's loose tree: the leaves on the paths become tight, an inner node on a path becomes the union of its children AS THEY ARE — a sibling off the
    # paths stays loose and so does what it reaches in its parent; off the paths nothing is tightened
    leaves = on_path & (old["count"] > 0)
    assert sparse[leaves].tobytes() == full[leaves].tobytes()
    for i in np.flatnonzero(on_path & (old["count"] == 0)):
        l, r = sparse["bounds"][old["first"][i]], sparse["bounds"][old["first"][i] + 1]
        want = np.empty(6, dtype=np.float32)
        want[0::2], want[1::2] = np.minimum(l[0::2], r[0::2]), np.maximum(l[1::2], r[1::2])
        assert sparse["bounds"][i].tobytes() == want.tobytes()
    assert sparse[~on_path].tobytes() != full[~on_path].tobytes() and sparse[on_path].tobytes() != full[on_path].tobytes()


def test_the_wrappers_refusals():
    """What Context.pose_parts refuses before the library sees it (scene.part_moves): a 4x4 matrix whose last row is not 0 0 0 1, a matrix of another shape, a
    negative first or count.  Ranges that overlap or leave the scene are the LIBRARY's to refuse — it names the positions (tests/test_pose_update.py) — so the
    Context wrapper does not check them; scene.pose_parts, the statement, and RVPT.pose_parts, which must keep its host copies right, do."""
    from rvpt_amd import native, scene
    eye = np.eye(4)
    bad_row = eye.copy()
    bad_row[3] = (0, 0, 0, 2)
    ctx = native.Context.__new__(native.Context)  # no library needed: the list is refused before any call
    for moves, what in (([(0, 1, bad_row)], "last row"), ([(0, 1, np.eye(3))], "3x4 or 4x4"), ([(-1, 1, eye)], "first = -1"), ([(0, -2, eye)], "count = -2"),
                        ([(2 ** 32, 1, eye)], "not a range")):
        with pytest.raises(ValueError, match=what):
            scene.part_moves(moves)
        with pytest.raises(native.NativeError, match=what) as e:
            native.Context.pose_parts(ctx, moves)
        assert e.value.code == native.ERR_INVALID
    assert native.Context.pose_parts(ctx, []) is None  # an empty list changes nothing and calls nothing
    tris = np.zeros((10, 16), dtype=np.float32)
    with pytest.raises(ValueError, match=r"moves\[1\] shares triangle 4"):
        scene.pose_parts(tris, [(2, 3, eye), (4, 2, eye)])
    with pytest.raises(ValueError, match=r"moves\[0\] = \[8, 8 \+ 3\) is outside the 10"):
        scene.pose_parts(tris, [(8, 3, eye)])
    with pytest.raises(ValueError, match="current has 9"):
        scene.pose_parts(tris, [(0, 1, eye)], current=tris[:9])


def test_part_move_from_a_rotation_and_a_translation():
    from rvpt_amd import scene
    r = rotation((1, 2, 3), 0.7)
    rec = scene.part_move(5, 9, rotation=r, translation=(1, -2, 3))
    assert rec.dtype == scene.PART_MOVE_DTYPE and rec["first"] == 5 and rec["count"] == 9 and not rec["reserved"].any()
    m = rec["m"].reshape(3, 4)
    assert m[:, :3].tobytes() == r.astype(np.float32).tobytes() and m[:, 3].tolist() == [1.0, -2.0, 3.0]
    assert scene.part_move(0, 1)["m"].reshape(3, 4).tolist() == np.eye(3, 4).tolist()


def test_the_mirror_splits_an_added_range_into_leaf_order_runs():
    """RVPT.pose_parts after a host build (no device: the context is a recorder): a range in the order the triangles were added goes down as one record per run
    of consecutive leaf-order positions, with the part's matrix, covering exactly the part's triangles; the host copies follow scene.pose_parts."""
    from rvpt_amd import RVPT, native, scene
    tris, mats = scene.default_scene()
    nodes, order = native.build_bvh(tris)
    order = np.asarray(order).astype(np.int64)

    class Recorder:
        def __init__(self):
            self.sent = []

        def pose_parts(self, rec):
            self.sent.append(np.array(rec, copy=True))

    r = RVPT(64, 48, traversal="bvh")
    r.add_triangles(tris)
    r._n_triangles, r._ctx = tris.shape[0], Recorder()
    r.bvh_nodes, r.primitive_indices, r.sorted_triangles = nodes, order, tris[order]
    m = about((0, 0, 2), rotation((0, 1, 0), 0.3))
    moves = [(10, 40, m), scene.part_move(100, 5, translation=(0, 0.5, 0))]
    assert r.pose_parts(moves) is None
    (sent,) = r._ctx.sent
    assert sent.dtype == native.PART_MOVE_DTYPE and not sent["reserved"].any() and (sent["count"] > 0).all()
    inverse = np.empty_like(order)
    inverse[order] = np.arange(order.size)
    for move in scene.part_moves(moves):
        mine = sent[(sent["m"] == move["m"]).all(axis=1)]
        covered = np.concatenate([np.arange(f, f + c) for f, c in zip(mine["first"], mine["count"])])
        assert sorted(covered.tolist()) == sorted(inverse[move["first"]:move["first"] + move["count"]].tolist())
    posed = scene.pose_parts(tris, moves)
    assert np.concatenate(r.triangles).tobytes() == posed.tobytes() and r.sorted_triangles.tobytes() == posed[order].tobytes()
    listed = inverse[np.concatenate([np.arange(10, 50), np.arange(100, 105)])]
    assert r.bvh_nodes.tobytes() == scene.refit_bvh(nodes, posed[order], touched=listed).tobytes()
    # a second pose of the first part starts from the rest pose; an update_triangles makes what the scene holds the new rest pose
    again = [(10, 40, about((0, 0, 2), rotation((0, 1, 0), -0.2)))]
    r.pose_parts(again)
    assert np.concatenate(r.triangles).tobytes() == scene.pose_parts(tris, again, current=posed).tobytes()
    for bad, what in (([(140, 4, m)], "outside the 143"), ([(0, 5, m), (4, 1, m)], "shares triangle 4"), ([(0, 0, m)], "count of 0"), ([(-1, 1, m)], "first = -1")):
        with pytest.raises(native.NativeError, match=what):
            r.pose_parts(bad)
    assert len(r._ctx.sent) == 2
