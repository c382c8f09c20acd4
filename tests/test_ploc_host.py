"""The PLOC tree of rvpt_hip_upload_scene's build form (RVPT_HIP_NODES_BUILD_PLOC), as numpy states it (rvpt_amd/scene.py: build_ploc; the definition is in
rvpt_amd/csrc/rvpt_build.h).  No GPU: tests/test_device_build_ploc.py compares the device's tree with this one bit for bit."""
import math

import numpy as np
import pytest

from rvpt_amd import scene
from rvpt_amd.scene import PLOC_MAX_HEIGHT, build_lbvh, build_ploc, refit_bvh
from test_lbvh_host import SCENES, check_tree


def box_tri(lo, hi):
    """a triangle whose box is [lo, hi]: two corners and a point between them"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return np.stack([lo, hi, (lo + hi) * np.float32(0.5)])


def tree_of(nodes, i=0):
    """the topology as nested tuples, a leaf as its sorted position"""
    if nodes[i]["count"] > 0:
        assert nodes[i]["count"] == 1
        return int(nodes[i]["first"])
    f = int(nodes[i]["first"])
    return (tree_of(nodes, f), tree_of(nodes, f + 1))


def sah_cost(nodes):
    """(sum of the inner nodes' half-areas + sum over the leaves of half-area x triangle count) / the root's half-area"""
    b = nodes["bounds"].astype(np.float64)
    e = b[:, 1::2] - b[:, 0::2]
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    total = 0.0
    stack = [0]
    while stack:
        i = stack.pop()
        if nodes[i]["count"] > 0:
            total += area[i] * int(nodes[i]["count"])
        else:
            total += area[i]
            stack += [int(nodes[i]["first"]), int(nodes[i]["first"]) + 1]
    return total / area[0]


@pytest.mark.parametrize("name", list(SCENES))
def test_build_ploc_gives_a_valid_tree(name):
    tris = np.ascontiguousarray(SCENES[name]())
    info = {}
    nodes, perm = build_ploc(tris, info=info)
    assert info["tree"] == "ploc"
    depth = check_tree(tris, nodes, perm, leaf_tris=1, finite=name != "nan_vertex")  # a permutation, one leaf per triangle, containment, children behind parents
    assert depth == info["height"] <= PLOC_MAX_HEIGHT
    n = tris.shape[0]
    assert np.array_equal(perm, build_lbvh(tris)[1])  # the LBVH's order
    # the layout: build_lbvh's, which is the device's (root 0, slot 1 unused, pairs on even indices) without the unused slot — upload_scene inserts it: root 0,
    # 2 n - 1 nodes, siblings adjacent, breadth first (the k-th inner node in index order owns the k-th pair)
    assert len(nodes) == 2 * n - 1
    inner = np.flatnonzero(nodes["count"] == 0)
    assert nodes["first"][inner].tolist() == list(range(1, 2 * n - 1, 2))
    assert nodes.tobytes() == refit_bvh(nodes, tris[perm]).tobytes()


def test_merges_on_a_line_written_down_by_hand():
    """Five triangles on the x axis with the boxes [0,1] [2,3] [4,5] [10,11] [12,13] (y, z extents 1, so d = 2 ex + 1): neighbours at distance
    d(0,1) = d(1,2) = d(3,4) = 7, d(0,2) = 11.  Iteration 1: cluster 1 is tied between 0 and 2 — 1 xor 0 = 1 beats 1 xor 2 = 3 — so (0,1) and (3,4) merge and
    2 stays.  Iteration 2 over A = [0,3], 2, B = [10,13]: d(A,2) = 11 beats d(2,B) = 19: (A,2).  Iteration 3: the root."""
    boxes = [(0, 1), (2, 3), (4, 5), (10, 11), (12, 13)]
    tris = scene.make_triangles(np.stack([box_tri((a, 0, 0), (b, 1, 1)) for a, b in boxes]), 0)
    info = {}
    nodes, perm = build_ploc(tris, info=info)
    assert perm.tolist() == [0, 1, 2, 3, 4] and info == {"tree": "ploc", "iterations": 3, "height": 4}
    assert tree_of(nodes) == (((0, 1), 2), (3, 4))
    # breadth first: root, [A2, B], [A, 2], [3, 4], [0, 1]
    assert nodes["first"].tolist() == [1, 3, 5, 7, 2, 3, 4, 0, 1] and nodes["count"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1]


def test_a_case_only_the_xor_term_decides():
    """Six IDENTICAL triangles: every distance is equal.  By (d, min(i, j)) alone every cluster i > 0 would
    choose 0 and only (0,1) would be mutual: a chain of height 6.  With the xor term the buddies pair up: (0,1) (2,3) (4,5), then 01 with 23 (0 xor 1 = 1 beats
    1 xor 2 = 3), 45 left over, then the root: height 4 in 3 iterations."""
    tris = np.repeat(scene.make_triangles(box_tri((0, 0, 0), (1, 1, 1))[None], 0), 6, axis=0)
    info = {}
    nodes, perm = build_ploc(tris, info=info)
    assert perm.tolist() == list(range(6)) and info == {"tree": "ploc", "iterations": 3, "height": 4}
    assert tree_of(nodes) == (((0, 1), (2, 3)), (4, 5))


def test_300_identical_triangles_pair_up_as_buddies():
    tris = np.repeat(scene.default_scene()[0][:1], 300, axis=0)
    info = {}
    nodes, perm = build_ploc(tris, info=info)
    print("300 identical triangles:", info)
    assert info["tree"] == "ploc"
    assert info["iterations"] <= math.ceil(math.log2(300)) + 1
    assert info["height"] <= 10


@pytest.mark.parametrize("name", ["default", "cornell", "heightfield64"])
def test_sah_cost_is_below_the_lbvhs(name):
    tris = {"default": scene.default_scene, "cornell": scene.cornell_scene, "heightfield64": lambda: scene.heightfield_scene(64)}[name]()[0]
    ploc, lbvh = sah_cost(build_ploc(tris)[0]), sah_cost(build_lbvh(tris)[0])
    print(f"{name}: SAH cost PLOC {ploc:.2f}, LBVH {lbvh:.2f}, ratio {ploc / lbvh:.3f}")
    assert ploc < lbvh


def nested_triangles(count=70, factor=1.3):
    """`count` copies of one triangle scaled about its centroid, the origin, each `factor` times the size of the last: all centroids coincide (exactly: the
    sums cancel in float32), so the caller's order is the leaf order, and every union box is the larger member's.  A cluster's candidates below it then all
    cost its own area, and only clusters 0 and 1 choose each other: each iteration merges one pair and the tree is a chain as high as the scene has triangles."""
    shape = np.array([[-1, 1, 0.5], [1, -0.5, -1], [0, -0.5, 0.5]], np.float32)
    p = np.stack([shape * s for s in (np.float32(factor) ** np.arange(count, dtype=np.float32))])
    return scene.make_triangles(p, 0)


def test_fallback_to_the_lbvh_tree():
    tris = nested_triangles()
    info = {}
    nodes, perm = build_ploc(tris, info=info)
    lbvh_nodes, lbvh_perm = build_lbvh(tris)
    check_tree(tris, lbvh_nodes, lbvh_perm)  # the LBVH of this input is legal
    assert info["tree"] == "lbvh" and info["height"] is None and info["iterations"] is not None  # finished, then found too high
    assert nodes.tobytes() == lbvh_nodes.tobytes() and np.array_equal(perm, lbvh_perm)
    # ... and one level less is a PLOC tree: the rule is the height, nothing about this input
    few = nested_triangles(PLOC_MAX_HEIGHT - 1)
    build_ploc(few, info=info)
    assert info["tree"] == "ploc" and info["height"] <= PLOC_MAX_HEIGHT


def test_the_tree_is_a_function_of_the_triangles():
    """Two runs give identical bytes; a shuffled input gives the same leaf-order triangles and the same nodes once the shuffle is undone (no two triangles of
    this heightfield share a Morton code)."""
    tris = scene.heightfield_scene(24)[0]
    nodes, perm = build_ploc(tris)
    again = build_ploc(tris.copy())
    assert nodes.tobytes() == again[0].tobytes() and np.array_equal(perm, again[1])
    shuffle = np.random.default_rng(5).permutation(tris.shape[0])
    nodes_s, perm_s = build_ploc(tris[shuffle])
    assert np.array_equal(shuffle[perm_s], perm) and nodes_s.tobytes() == nodes.tobytes()
    fall = nested_triangles()
    assert build_ploc(fall)[0].tobytes() == build_ploc(fall.copy())[0].tobytes()
