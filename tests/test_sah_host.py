"""The SAH tree of rvpt_hip_upload_scene's SAH build form, as numpy states it (rvpt_amd/scene.py: build_sah; the definition is "THE SAH TREE" in
rvpt_amd/csrc/rvpt_build.h), and the claim that it is rvpt_bvh_build's tree node for node.  No GPU: tests/test_device_build_sah.py compares the device's tree
with this one bit for bit."""
import numpy as np
import pytest

import _device_state as ds
from rvpt_amd import scene
from rvpt_amd.scene import build_sah
from test_lbvh_host import SCENES, scene_of, strip


def check_sah_tree(tris, nodes, perm, info, finite=True):
    """a permutation; every triangle in exactly one leaf; leaves of 1 .. 8; containment; the breadth-first layout (children adjacent, the pairs of a level in
    the order of their parents, levels one after the other); height <= 30 + ceil(log2 n) + 1; boxes == refit_bvh byte for byte.  Returns the height."""
    n = tris.shape[0]
    assert nodes.dtype == scene.NODE_DTYPE and perm.dtype == np.uint32
    assert sorted(perm.tolist()) == list(range(n))
    st = tris[perm]
    first, count = nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    seen = np.zeros(n, dtype=np.int32)
    level, height, next_index, max_leaf = np.zeros(1, dtype=np.int64), 0, 1, 0
    while level.size:
        height += 1
        inner = level[count[level] == 0]
        leaves = level[count[level] > 0]
        for i in leaves:
            f, c = int(first[i]), int(count[i])
            assert 1 <= c <= scene.SAH_MAX_LEAF
            max_leaf = max(max_leaf, c)
            seen[f:f + c] += 1
            if finite:
                p = st[f:f + c][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
                b = nodes[i]["bounds"]
                assert (p >= b[0::2]).all() and (p <= b[1::2]).all()
        assert np.array_equal(first[inner], next_index + 2 * np.arange(inner.size))  # the k-th splitting node of the level owns the pair next_begin + 2 k
        if finite:
            for i in inner:
                b = nodes[i]["bounds"]
                for ch in (first[i], first[i] + 1):
                    cb = nodes[ch]["bounds"]
                    assert (cb[0::2] >= b[0::2]).all() and (cb[1::2] <= b[1::2]).all()
        next_index += 2 * inner.size
        level = np.stack([first[inner], first[inner] + 1], axis=1).reshape(-1)
    assert next_index == len(nodes) and (seen == 1).all()
    assert height <= 30 + int(np.ceil(np.log2(n))) + 1
    assert info["height"] == height and info["max_leaf"] == max_leaf
    assert info["binned_splits"] + info["median_splits"] == (len(nodes) - 1) // 2
    if finite:
        assert nodes.tobytes() == scene.refit_bvh(nodes, st).tobytes()
    return height


@pytest.mark.parametrize("name", list(SCENES))
def test_build_sah_gives_a_valid_tree(name):
    tris = np.ascontiguousarray(SCENES[name]())
    nodes, perm, info = build_sah(tris)
    check_sah_tree(tris, nodes, perm, info, finite=name != "nan_vertex")
    again = build_sah(tris.copy())
    assert nodes.tobytes() == again[0].tobytes() and np.array_equal(perm, again[1]) and info == again[2]
    if tris.shape[0] < scene.SAH_MIN_LEAF:
        assert len(nodes) == 1 and nodes[0]["count"] == tris.shape[0]


def same_tree(a, pa, b, pb):
    """both trees walked from the root, left with left and right with right: equal leaf / inner shape, equal bounds bytes, equal SETS of caller's indices"""
    stack, visited = [(0, 0)], 0
    while stack:
        i, j = stack.pop()
        visited += 1
        x, y = a[i], b[j]
        assert x["count"] == y["count"], f"nodes {i} / {j}: {x['count']} against {y['count']} triangles"
        assert x["bounds"].tobytes() == y["bounds"].tobytes(), f"nodes {i} / {j}: {x['bounds']} against {y['bounds']}"
        if x["count"] > 0:
            assert set(pa[x["first"]:x["first"] + x["count"]].tolist()) == set(pb[y["first"]:y["first"] + y["count"]].tolist()), f"leaves {i} / {j}"
        else:
            stack.append((int(x["first"]), int(y["first"])))
            stack.append((int(x["first"]) + 1, int(y["first"]) + 1))
    assert visited == len(a) == len(b)


HOST_SCENES = {k: v for k, v in SCENES.items() if k != "nan_vertex"}  # (the host's float-to-int conversion of a NaN is undefined)
HOST_SCENES["heightfield66k"] = lambda: scene.heightfield_scene(182)[0]  # above 32 768 triangles: the host builder's threaded path


@pytest.mark.parametrize("name", list(HOST_SCENES))
def test_build_sah_is_the_host_builders_tree(name):
    """The claim of the SAH build form: node for node the triangle sets and the boxes are rvpt_bvh_build's."""
    from rvpt_amd import native
    tris = np.ascontiguousarray(HOST_SCENES[name]())
    nodes, perm, _ = build_sah(tris)
    host_nodes, host_perm = native.build_bvh(tris)
    same_tree(nodes, perm, host_nodes.view(scene.NODE_DTYPE).reshape(-1), host_perm)


def test_two_triangles():
    """Centroids at x = 0 and x = 1 (points): bins 0 and 15 on axis 0, every candidate split costs 0 + 0, the leaf 0 * 2 = 0: 0 < 0 fails and two triangles
    are a leaf.  With an extent in y the leaf costs area * 2 > the split's two smaller areas: one binned split."""
    nodes, perm, info = build_sah(scene_of([(0, 0, 0), (1, 0, 0)]))
    assert len(nodes) == 1 and nodes[0]["count"] == 2 and info == {"height": 1, "binned_splits": 0, "median_splits": 0, "max_leaf": 2}
    nodes, perm, info = build_sah(strip(2))
    assert nodes["count"].tolist() == [0, 1, 1] and perm.tolist() == [0, 1] and info["binned_splits"] == 1 and info["height"] == 2


def collinear9():
    """nine triangles (0,0,0) (1,0,0) (0,1,0.5) shifted to x = 0, 1, 2, 3, 4, 5, 6, 7, 16"""
    x = np.array([0, 1, 2, 3, 4, 5, 6, 7, 16], dtype=np.float32)[:, None, None]
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)[None] + x * np.array([1, 0, 0], np.float32)
    return scene.make_triangles(p, 0)


def test_nine_collinear_triangles():
    """Centroid x = k + 1/3 for k = 0 .. 7 and 16 + 1/3: extent 16, scale 1, bins 0 .. 7 and 15; y and z have no extent, so axis 0 alone is swept.  Every box
    is dy = 1, dz = 0.5 with dx = its span: half_area = dx * 1.5 + 0.5.  Splitting in front of bin b (b = 1 .. 8 differ; 9 .. 15 equal 8): left holds b
    triangles spanning dx = b, right 9 - b spanning 17 - b:
        cost(b) = (1.5 b + 0.5) b + (1.5 (17 - b) + 0.5) (9 - b),   b = 1 .. 7   ->  198, 168, 144, 126, 114, 108, 108
        cost(8) = (1.5 * 8 + 0.5) * 8 + (1.5 * 1 + 0.5) * 1 = 102, and the same for b = 9 .. 15 (the same sets).
    The first strict minimum is (axis 0, bin 8): the eight near triangles go left, the far one right; leaf cost (1.5 * 17 + 0.5) * 9 = 234 > 102."""
    nodes, perm, info = build_sah(collinear9())
    assert nodes[0]["count"] == 0 and perm[8] == 8
    left, right = nodes[int(nodes[0]["first"])], nodes[int(nodes[0]["first"]) + 1]
    assert right["count"] == 1 and right["first"] == 8 and left["count"] == 0
    assert left["bounds"][0] == 0 and left["bounds"][1] == 8


def test_axes_that_tie_give_axis_zero():
    """Four point triangles on the diagonal of a square, (0,0) (1,1) (2,2) (3,3) in x and y, with a spread in x and y alike (size on both): every candidate of
    axis 1 costs exactly what the same candidate of axis 0 costs, and strict < keeps axis 0.  The partition by x alone and by y alone would give the same sets
    here, so the order tells: a scene mirrored in y (y = 3 - x) has the same costs and must still split by x — left = the small x."""
    def tri(x, y):
        return np.array([[x - 0.25, y - 0.25, 0], [x + 0.25, y, 0], [x, y + 0.25, 0]], np.float32)
    tris = scene.make_triangles(np.stack([tri(x, 3 - x) for x in (3, 1, 0, 2)]), 0)
    nodes, perm, info = build_sah(tris)
    first = int(nodes[0]["first"])
    assert nodes[0]["count"] == 0 and info["median_splits"] == 0
    xs = tris[perm][:, 0]
    n_left = int(nodes[first]["count"]) or 2
    assert xs[:n_left].max() < xs[n_left:].min()  # by x: left is the small x (by y it would be the large x)
    assert nodes[first]["bounds"][1] <= nodes[first + 1]["bounds"][0] + 0.5


def test_identical_triangles_take_median_splits_by_index():
    """300 identical triangles: no centroid extent, nothing to bin; 300 > 8 -> the median split, its sort decided by the caller's index alone: perm is the
    identity, and 300 -> 150 -> 75 -> 37 | 38 -> 18 | 19 -> 9 | 10 -> 4 | 5: leaves on level 7."""
    tris = np.repeat(scene.default_scene()[0][:1], 300, axis=0)
    nodes, perm, info = build_sah(tris)
    assert info["median_splits"] > 0 and info["binned_splits"] == 0
    assert perm.tolist() == list(range(300)) and info["height"] == 7 and info["max_leaf"] == 5


def test_median_split_decided_by_the_index_tie_break():
    """Twelve point triangles at the SAME place: nothing to bin, 12 > 8, every (NaN, value) key ties and the caller's index alone orders the range — the left
    child takes indices 0 .. 5.  Then ten points of which two lie at x = 1: point boxes have half_area 0, no split beats the leaf cost 0 (0 < 0 fails), 10 > 8:
    the median sort puts the value first and the index second."""
    tris = np.repeat(scene_of([(1, 2, 3)]), 12, axis=0)
    nodes, perm, info = build_sah(tris)
    first = int(nodes[0]["first"])
    assert info["median_splits"] == 1 and info["binned_splits"] == 0
    assert nodes[first]["count"] == 6 and nodes[first + 1]["count"] == 6 and perm.tolist() == list(range(12))
    cents = [(0, 0, 0)] * 4 + [(1, 0, 0)] * 2 + [(0, 0, 0)] * 4
    nodes, perm, info = build_sah(scene_of(cents))
    assert info["median_splits"] == 1 and sorted(perm[:5].tolist()) == [0, 1, 2, 3, 6] and perm[:5].tolist() == [0, 1, 2, 3, 6]  # value first, then index
    assert perm[5:].tolist() == [7, 8, 9, 4, 5]


def test_negative_zero_equals_zero_in_the_median_sort():
    """Ten point triangles whose centroid x is +0 and -0 alternately, y = z = 0: all three extents are 0, axis 0 is the widest (the first strict maximum from
    -1), and -0 == +0 leaves the index to decide — an order that told the zeros apart would put the odd indices first."""
    cents = [(-0.0 if k % 2 else 0.0, 0, 0) for k in range(10)]
    tris = scene_of(cents)
    assert np.signbit(tris[1, 0]) and not np.signbit(tris[0, 0])
    nodes, perm, info = build_sah(tris)
    assert info["median_splits"] == 1 and perm.tolist() == list(range(10))


@pytest.mark.parametrize("k", [0, 3])
def test_the_depth_rule(k):
    """balance_depth = k on strip2000: from level k on only median splits (no binning), and the tree stays valid.  The device's trigger is the same comparison
    against the compile-time 30 (rv::kSahBalanceDepth); the bins halve well-spread scenes long before depth 30, so the GPU meets that branch of the kernels on
    tests/_device_state.py's geometric ladder alone: test_the_ladder_reaches_the_depth_rule below states its trees, tests/test_device_state.py's ladder
    tests compare the device's with them byte for byte, and tests/test_ray_query.py walks one."""
    tris = strip(2000)
    nodes, perm, info = build_sah(tris, balance_depth=k)
    check_sah_tree(tris, nodes, perm, info)
    full = build_sah(tris)
    assert info["median_splits"] > 0
    # the splits of the levels above k are the binned ones of the ordinary tree
    first, count = nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    level, depth, binned_above = np.zeros(1, dtype=np.int64), 0, 0
    while level.size and depth < k:
        inner = level[count[level] == 0]
        binned_above += inner.size
        level = np.stack([first[inner], first[inner] + 1], axis=1).reshape(-1)
        depth += 1
    assert info["binned_splits"] == binned_above and info["binned_splits"] + info["median_splits"] == (len(nodes) - 1) // 2
    assert full[2]["median_splits"] == 0
    # a median split halves: below level k the tree is balanced, leaves of <= 8
    assert info["height"] <= k + int(np.ceil(np.log2(2000))) + 1


@pytest.mark.parametrize("row", list(ds.LADDERS), ids=["-".join(map(str, r)) for r in ds.LADDERS])
def test_the_ladder_reaches_the_depth_rule(row):
    """tests/_device_state.py's geometric ladder: the binned split peels one triangle per level down to depth 30 (rv::kSahBalanceDepth), where the cluster
    arrives whole and takes median splits only.  The builder's report is the table's, exactly; every level that still holds a rung has one inner node, with a
    child of one triangle; every inner node from depth 30 on has children whose counts differ by at most one; and the tree is rvpt_bvh_build's.  The row of 29
    rungs has one more inner node above depth 30, the cluster itself at depth 29: no rung is left to peel, its split is binned all the same (156 | 144)."""
    from rvpt_amd import native
    want = ds.LADDERS[row]
    tris = ds.ladder(*row)
    assert tris.shape[0] == want["n"] and ds.no_zero_coordinate(tris)
    c = (tris[:, 0:3] + tris[:, 4:7] + tris[:, 8:11]) * np.float32(1.0 / 3.0)
    assert np.ptp(c[:, 1]) == 0 and np.ptp(c[:, 2]) == 0 and np.unique(c[:, 0]).size == want["n"]  # one live axis, no two centroids alike
    nodes, perm, info = build_sah(tris)
    assert check_sah_tree(tris, nodes, perm, info) == want["height"]
    assert info == {k: v for k, v in want.items() if k != "n"}
    first, count = nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    below = np.zeros(len(nodes), dtype=np.int64)  # triangles below every node: children follow their parents in the layout
    for i in range(len(nodes) - 1, -1, -1):
        below[i] = count[i] if count[i] > 0 else below[first[i]] + below[first[i] + 1]
    level, depth, binned, medians = np.zeros(1, dtype=np.int64), 0, 0, 0
    while level.size:
        inner = level[count[level] == 0]
        left, right = below[first[inner]], below[first[inner] + 1]
        if depth < row[0]:  # a rung is still there
            assert inner.size == 1 and ((left == 1) | (right == 1)).all(), depth
            binned += inner.size
        elif depth < scene.SAH_BALANCE_DEPTH:  # (29, 300, 3): the cluster's first split is still a binned one, by the bins' cost and not in halves
            assert inner.size == 1 and (np.abs(left - right) > 1).all(), (depth, left, right)
            binned += inner.size
        else:
            assert (np.abs(left - right) <= 1).all(), depth
            medians += inner.size
        level = np.stack([first[inner], first[inner] + 1], axis=1).reshape(-1)
        depth += 1
    assert (binned, medians) == (want["binned_splits"], want["median_splits"])
    host_nodes, host_perm = native.build_bvh(tris)
    same_tree(nodes, perm, host_nodes.view(scene.NODE_DTYPE).reshape(-1), host_perm)


def infinite_axis(n=12):
    """n triangles whose x coordinates are all +inf, y falling with the index, z constant"""
    p = np.zeros((n, 3, 3), np.float32)
    p[:, :, 0] = np.inf
    p[:, :, 1] = (np.arange(n, 0, -1, dtype=np.float32) * 1.5)[:, None] + np.array([0.25, 0.5, 0.75], np.float32)
    p[:, :, 2] = np.array([1.25, 1.5, 1.75], np.float32)
    with np.errstate(all="ignore"):
        return scene.make_triangles(p, 0)


def test_a_low_side_of_nothing_but_infinity_is_flt_max_as_in_the_hosts_box():
    """bvh_builder.cpp's Box starts at +-FLT_MAX and takes std::min / std::max: the centroid bounds of a node whose x centroids are all +inf are [FLT_MAX, +inf],
    extent +inf, so x is the widest axis and the median split sorts by (x: all equal, index): the left child takes the first half of the caller's order.  With
    lo = +inf the extent would be a NaN, y the widest axis, and the left child the LAST half (y falls with the index)."""
    tris = infinite_axis()
    with np.errstate(all="ignore"):
        nodes, perm, info = build_sah(tris)
    assert info["median_splits"] >= 1 and nodes[0]["count"] == 0
    left = nodes[nodes[0]["first"]]
    assert left["count"] == 6 and sorted(perm[left["first"]: left["first"] + 6].tolist()) == [0, 1, 2, 3, 4, 5]
