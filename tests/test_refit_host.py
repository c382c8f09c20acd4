"""The normative refit of a tree whose triangles moved (rvpt_amd/scene.py: refit_bvh — the host statement of what the update form of rvpt_hip_upload_scene
does on the device), GPU-free: it reproduces the builder's boxes byte for byte, keeps the topology, and its boxes contain what they must."""
import numpy as np
import pytest

from rvpt_amd import native, scene

SCENES = {"default": scene.default_scene, "cornell": scene.cornell_scene, "terrain64": lambda: scene.heightfield_scene(64)}


def _built(name):
    tris, _ = SCENES[name]()
    nodes, idx = native.build_bvh(tris)
    return nodes, tris[idx]


def _extent(tris):
    return float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())


def _head_shift(n_nodes, n_tris):
    """upload_scene's rule: indices of the device layout (one slot more than the caller's nodes) and of the triangles below 2^shift"""
    shift = 1
    while (1 << shift) <= max(n_nodes + 1, n_tris):
        shift += 1
    return shift


@pytest.mark.parametrize("name", sorted(SCENES))
def test_refit_of_unmoved_triangles_is_the_builders_tree(name):
    """The builder's boxes are tight, min / max is exact: "update with the same vertices" must leave every node as it was, byte for byte."""
    nodes, tris = _built(name)
    again = scene.refit_bvh(nodes, tris)
    assert again.dtype == nodes.dtype and again.shape == nodes.shape
    assert again.tobytes() == nodes.tobytes()
    rec = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)  # the record form goes in and comes out as records
    assert scene.refit_bvh(rec, tris).tobytes() == nodes.tobytes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_refit_after_a_deformation(name):
    """Every box contains its children's boxes and its triangles' vertices and is tight (some vertex lies on each face), `first` / `count` are unchanged.

    The wide form: the device keeps the grouping it chose at the full upload (exact for any tree whose boxes contain their children, which a refit guarantees);
    a FRESH regrouping of the refit tree may group differently, because build_wide_nodes opens the child with the largest box first and the deformation
    changes the areas.  This test checks that documented case: the fresh regrouping's heads equal the old ones, or — where the heuristic chose otherwise —
    both list exactly the same leaves (the leaf heads are a function of the topology alone)."""
    nodes, tris = _built(name)
    moved = scene.wobble(tris, 0.8, 0.1 * _extent(tris))
    assert not np.array_equal(moved, tris) and np.array_equal(moved[:, 12:], tris[:, 12:])
    refit = scene.refit_bvh(nodes, moved)
    a, b = nodes.view(native.NODE_DTYPE).reshape(-1), refit.view(native.NODE_DTYPE).reshape(-1)
    assert np.array_equal(a["first"], b["first"]) and np.array_equal(a["count"], b["count"])
    assert not np.array_equal(a["bounds"], b["bounds"])
    lo, hi = b["bounds"][:, 0::2], b["bounds"][:, 1::2]
    inner = np.flatnonzero(b["count"] == 0)
    for c in (b["first"][inner], b["first"][inner] + 1):
        assert (lo[c] >= lo[inner]).all() and (hi[c] <= hi[inner]).all()
    assert np.array_equal(np.minimum(lo[b["first"][inner]], lo[b["first"][inner] + 1]), lo[inner])
    assert np.array_equal(np.maximum(hi[b["first"][inner]], hi[b["first"][inner] + 1]), hi[inner])
    v = moved.reshape(-1, 4, 4)[:, :3, :3]
    for i in np.flatnonzero(b["count"] > 0):
        p = v[b["first"][i]: b["first"][i] + b["count"][i]].reshape(-1, 3)
        assert np.array_equal(p.min(axis=0), lo[i]) and np.array_equal(p.max(axis=0), hi[i])
    shift = _head_shift(len(a), tris.shape[0])
    before, need0 = native.wide_form(nodes, shift)
    after, need1 = native.wide_form(refit, shift)
    h0, h1 = before[:, 6, :].view(np.uint32), after[:, 6, :].view(np.uint32)
    if not (h0.shape == h1.shape and np.array_equal(h0, h1)):
        leaf = lambda h: np.sort(h[(h != 0xFFFFFFFF) & ((h >> shift) > 0)])
        assert np.array_equal(leaf(h0), leaf(h1))


def test_refit_tightens_loose_boxes_and_rejects_what_is_not_a_tree():
    nodes, tris = _built("default")
    rec = nodes.view(native.NODE_DTYPE).reshape(-1).copy()
    inner = np.flatnonzero(rec["count"] == 0)
    rec["bounds"][inner[::2], 0::2] -= 0.5  # grown
    rec["bounds"][inner[1::2], 1::2] -= 0.01  # shrunk: no longer contains its children
    assert scene.refit_bvh(rec, tris).tobytes() == nodes.tobytes()
    bad = nodes.copy()
    bad.view(native.NODE_DTYPE).reshape(-1)["first"][inner[-1]] = len(rec)  # a child outside the array
    with pytest.raises(ValueError):
        scene.refit_bvh(bad, tris)
    loop = nodes.copy()
    loop.view(native.NODE_DTYPE).reshape(-1)["first"][inner[-1]] = 0  # back to the root
    with pytest.raises(ValueError):
        scene.refit_bvh(loop, tris)
    short = nodes.copy()
    with pytest.raises(ValueError):
        scene.refit_bvh(short, tris[:-1])


def test_wobble_keeps_shared_vertices_welded():
    tris, _ = scene.heightfield_scene(8)
    moved = scene.wobble(tris, 1.1, 0.3)
    p0, p1 = tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), moved.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3)
    _, inverse = np.unique(p0, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for g in range(int(inverse.max()) + 1):
        q = p1[inverse == g]
        assert (q == q[0]).all()
    assert np.abs(p1 - p0).max() <= 0.3 * 1.0001


def test_renderer_and_context_check_their_arguments_without_a_gpu():
    """Shape / dtype / order-of-calls checks that need no device (the context itself is never made here)."""
    from rvpt_amd import RVPT
    r = RVPT(32, 32, traversal="bvh")
    with pytest.raises(RuntimeError):
        r.update_triangles(np.zeros((3, 16), np.float32))
    nodes, tris = _built("default")
    r.bvh_nodes, r.sorted_triangles = nodes, scene.wobble(tris, 0.3, 0.2)
    assert r.bvh_nodes is nodes  # a plain assignment is what it was
    r._nodes_stale = True  # what update_triangles leaves behind: refitted on demand, once
    first = r.bvh_nodes
    assert first.tobytes() == scene.refit_bvh(nodes, r.sorted_triangles).tobytes() and r.bvh_nodes is first


def _slow_refit(nodes, tris):
    """refit_bvh's rule said once more, one node and one coordinate at a time, in Python floats: a bound is the min / max of the values that are not NaN, and
    NaN where there is none"""
    import math
    rec = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1).copy()
    v = tris.reshape(-1, 4, 4)[:, :3, :3]

    def fold(values, pick):
        real = [float(x) for x in values if not math.isnan(x)]
        return pick(real) if real else math.nan

    def visit(i):
        f, c = int(rec["first"][i]), int(rec["count"][i])
        if c > 0:
            los = his = [v[f:f + c, :, ax].reshape(-1).tolist() for ax in range(3)]
        else:
            visit(f), visit(f + 1)
            los = [[rec["bounds"][f][2 * ax], rec["bounds"][f + 1][2 * ax]] for ax in range(3)]
            his = [[rec["bounds"][f][2 * ax + 1], rec["bounds"][f + 1][2 * ax + 1]] for ax in range(3)]
        for ax in range(3):
            rec["bounds"][i][2 * ax], rec["bounds"][i][2 * ax + 1] = fold(los[ax], min), fold(his[ax], max)

    visit(0)
    return rec


def _same_with_nan_in_place(a, b):
    a, b = a["bounds"], b["bounds"]
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _non_finite_soup(n, seed, whole_axis=None):
    rng = np.random.RandomState(seed)
    p = (rng.uniform(-4, 4, (n, 1, 3)) + rng.uniform(-0.3, 0.3, (n, 3, 3))).astype(np.float32)
    pick = rng.permutation(n)[:max(3, n // 50)]
    for j, i in enumerate(pick):
        val = (np.nan, np.inf, -np.inf)[j % 3]
        if (j // 3) % 2 == 0:
            p[i, rng.randint(3), rng.randint(3)] = val
        else:
            p[i] = val
    if whole_axis is not None:
        p[:, :, whole_axis] = np.nan
    with np.errstate(all="ignore"):
        return scene.make_triangles(p, 0), pick


@pytest.mark.parametrize("builder", ["lbvh", "ploc", "sah"])
@pytest.mark.parametrize("n,axis", [(65, None), (257, 1), (1025, None)])
def test_a_nan_takes_no_part_in_a_refit(builder, n, axis):
    """rvpt_build.h's rule, which the device's fminf / fmaxf follow: a NaN coordinate takes no part in a box; a bound is NaN only where nothing else took part
    (a whole leaf's coordinates on an axis, both children's bounds); infinities are ordinary values.  The full refit, the sparse form, and the boxes the three
    numpy builders return (they end in refit_bvh) against the rule said one coordinate at a time."""
    tris, pick = _non_finite_soup(n, 100 + n, axis)
    with np.errstate(all="ignore"):
        nodes, perm = {"lbvh": scene.build_lbvh, "ploc": scene.build_ploc, "sah": scene.build_sah}[builder](tris)[:2]
    t = tris[perm]
    want = _slow_refit(nodes, t)
    assert _same_with_nan_in_place(nodes, want)
    b = nodes["bounds"]
    if axis is None:
        assert not np.isnan(b[0]).any()  # the root: finite triangles took part on every axis ...
        assert np.isinf(b[0]).any()       # ... and so did the infinities
        # a finite triangle that shares a leaf with a NaN one is not hidden: no leaf bound is NaN unless the whole leaf is NaN on that axis
        v = t.reshape(-1, 4, 4)[:, :3, :3]
        for i in np.flatnonzero(nodes["count"] > 0):
            p = v[nodes["first"][i]: nodes["first"][i] + nodes["count"][i]].reshape(-1, 3)
            assert np.array_equal(np.isnan(b[i][0::2]), np.isnan(p).all(axis=0)) and np.array_equal(np.isnan(b[i][1::2]), np.isnan(p).all(axis=0))
    else:
        assert np.isnan(b[:, 2 * axis: 2 * axis + 2]).all() and not np.isnan(np.delete(b[0], [2 * axis, 2 * axis + 1])).any()
    # the sparse form: move the non-finite values elsewhere, touch both sets
    moved, pick2 = _non_finite_soup(n, 200 + n, axis)
    moved = moved[perm]
    inv = np.argsort(perm)
    touched = np.unique(np.concatenate([inv[pick], inv[pick2]]))
    patched = t.copy()
    patched[touched] = moved[touched]
    with np.errstate(all="ignore"):
        sparse, full = scene.refit_bvh(nodes, patched, touched=touched), scene.refit_bvh(nodes, patched)
    assert _same_with_nan_in_place(full, _slow_refit(nodes, patched))
    assert _same_with_nan_in_place(sparse, full)  # the boxes were tight: the sparse refit is the full one


def test_finite_triangles_refit_to_the_bytes_of_plain_min_and_max():
    """... and without a NaN nothing changed: the boxes are ndarray.min / max and np.minimum / np.maximum of before, zeros of either sign included"""
    tris, _ = scene.heightfield_scene(16)
    tris = tris.copy()
    tris[::5, 0] = -0.0
    tris[1::7, 1] = 0.0
    tris[2::9, 6] = np.inf
    nodes, perm = scene.build_lbvh(tris)
    t = tris[perm]
    v = t.reshape(-1, 4, 4)[:, :3, :3]
    tlo, thi = v.min(axis=1), v.max(axis=1)
    old = nodes.copy()
    for i in reversed(range(len(old))):  # breadth first: children behind their parent
        f, c = int(old["first"][i]), int(old["count"][i])
        if c > 0:
            lo, hi = tlo[f], thi[f]
            for k in range(1, c):
                lo, hi = np.minimum(lo, tlo[f + k]), np.maximum(hi, thi[f + k])
        else:
            lo, hi = np.minimum(old["bounds"][f][0::2], old["bounds"][f + 1][0::2]), np.maximum(old["bounds"][f][1::2], old["bounds"][f + 1][1::2])
        old["bounds"][i][0::2], old["bounds"][i][1::2] = lo, hi
    assert scene.refit_bvh(nodes, t).tobytes() == old.tobytes()
    pos = np.arange(0, t.shape[0], 3)
    assert scene.refit_bvh(nodes, t, touched=pos).tobytes() == old.tobytes()
