"""The LBVH of rvpt_hip_upload_scene's build form, as numpy states it (rvpt_amd/scene.py: lbvh_keys, build_lbvh; the definition is in
rvpt_amd/csrc/rvpt_build.h).  No GPU: tests/test_device_build.py compares the device's tree with this one bit for bit."""
import numpy as np
import pytest

from rvpt_amd import scene
from rvpt_amd.scene import LBVH_LEAF_TRIS, build_lbvh, lbvh_keys


def tri_at(c, size=0.0):
    """a triangle whose three vertices are c (+ a spread that keeps the centroid: -size, 0, +size on x)"""
    c = np.asarray(c, dtype=np.float32)
    p = np.stack([c, c, c]).astype(np.float32)
    p[0, 0] -= size
    p[2, 0] += size
    return p


def scene_of(centroids):
    return scene.make_triangles(np.stack([tri_at(c) for c in centroids]), 0)


def codes(tris):
    k = lbvh_keys(tris)
    assert np.array_equal(k & np.uint64(0xFFFFFFFF), np.arange(len(k), dtype=np.uint64))  # the caller's index rides below the code
    return (k >> np.uint64(32)).astype(np.int64)


def interleave(qx, qy, qz):
    code = 0
    for b in range(10):
        code |= ((qx >> b) & 1) << (3 * b + 2) | ((qy >> b) & 1) << (3 * b + 1) | ((qz >> b) & 1) << (3 * b)
    return code


def test_key_interleave_order_and_clamp():
    """Centroid bounds [0, 1024]^3: scale 1, q = (int)c, the far corner clamps to 1023; x is the highest bit of every triple."""
    cents = [(0, 0, 0), (1024, 1024, 1024), (1, 0, 0), (0, 1, 0), (0, 0, 1), (512, 0, 0), (0, 512, 0), (0, 0, 512), (3, 5, 6), (1023.5, 2.75, 1000.25)]
    got = codes(scene_of(cents))
    want = [interleave(0, 0, 0), interleave(1023, 1023, 1023), 4, 2, 1, 1 << 29, 1 << 28, 1 << 27, interleave(3, 5, 6), interleave(1023, 2, 1000)]
    assert got.tolist() == want
    assert got[1] == (1 << 30) - 1


def test_key_quantisation_is_float32():
    """q = (int)((c - lo) * (1024.0f / (hi - lo))) in float32: bounds [0, 3] give the scale 341.33334f; 3 * 341.33334f = 1024.00003 clamps to 1023,
    1.5 -> 512.00002 -> 512, 2.25 -> 768.00002 -> 768, 1 -> 341, 0.01 -> 3.41 -> 3."""
    cents = [(0, 0, 0), (3, 0, 0), (1.5, 0, 0), (2.25, 0, 0), (1, 0, 0), (0.01, 0, 0)]
    got = codes(scene_of(cents))
    assert got.tolist() == [interleave(q, 0, 0) for q in (0, 1023, 512, 768, 341, 3)]  # y and z have no extent: q = 0


def test_key_zero_extent_axis_and_nan():
    """An axis whose extent is not > 0 gives q = 0 for everyone; a NaN centroid takes no part in the bounds and gets q = 0 on its axis."""
    cents = [(0, 7, 0), (2, 7, 4), (1, 7, 2), (np.nan, 7, 4)]
    got = codes(scene_of(cents))
    assert got.tolist() == [interleave(0, 0, 0), interleave(1023, 0, 1023), interleave(512, 0, 512), interleave(0, 0, 1023)]
    assert codes(scene_of([(np.nan, np.nan, np.nan)] * 3)).tolist() == [0, 0, 0]
    assert codes(scene_of([(np.inf, 0, 0), (0, 0, 0), (1, 0, 0)])).tolist() == [0, 0, 0]  # extent inf: the scale is 0, and inf * 0 is a NaN


def check_tree(tris, nodes, perm, leaf_tris=LBVH_LEAF_TRIS, finite=True):
    """The criteria of check_bvh (tests/test_abi_exports.py) — a permutation, every triangle in exactly one leaf, containment, depth <= 62 — plus the LBVH's own:
    leaves of 1 .. leaf_tris triangles, no inner node that would fit a leaf, children adjacent and behind their parent."""
    n = tris.shape[0]
    assert nodes.dtype == scene.NODE_DTYPE and perm.dtype == np.uint32
    assert sorted(perm.tolist()) == list(range(n))
    st = tris[perm]
    seen = np.zeros(n, dtype=np.int32)
    visited = np.zeros(len(nodes), dtype=np.int32)
    max_depth, stack = 0, [(0, 1)]
    sizes = {}

    def size_of(i):
        if i not in sizes:
            sizes[i] = int(nodes[i]["count"]) if nodes[i]["count"] > 0 else size_of(int(nodes[i]["first"])) + size_of(int(nodes[i]["first"]) + 1)
        return sizes[i]

    while stack:
        i, depth = stack.pop()
        visited[i] += 1
        max_depth = max(max_depth, depth)
        b = nodes[i]["bounds"]
        if nodes[i]["count"] > 0:
            f, c = int(nodes[i]["first"]), int(nodes[i]["count"])
            assert 1 <= c <= leaf_tris
            seen[f:f + c] += 1
            if finite:
                p = st[f:f + c][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3)
                assert (p >= b[0::2]).all() and (p <= b[1::2]).all()
        else:
            l = int(nodes[i]["first"])
            assert i < l and l + 1 < len(nodes)
            for ch in (l, l + 1):
                if finite:
                    cb = nodes[ch]["bounds"]
                    assert (cb[0::2] >= b[0::2]).all() and (cb[1::2] <= b[1::2]).all()
                stack.append((ch, depth + 1))
    assert (seen == 1).all() and (visited == 1).all()
    assert all(size_of(i) > leaf_tris for i in range(len(nodes)) if nodes[i]["count"] == 0)
    assert max_depth <= 62
    return max_depth


def strip(n):
    """n triangles in a row along x"""
    x = np.arange(n, dtype=np.float32)[:, None, None]
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)[None] + x * np.array([1, 0, 0], np.float32)
    return scene.make_triangles(p, 0)


def nan_scene():
    tris, _ = scene.default_scene()
    tris = tris.copy()
    tris[17, 5] = np.nan
    return tris


SCENES = {
    "default": lambda: scene.default_scene()[0],
    "one": lambda: scene.default_scene()[0][:1],
    "n_le_L": lambda: scene.default_scene()[0][:LBVH_LEAF_TRIS],
    "identical300": lambda: np.repeat(scene.default_scene()[0][:1], 300, axis=0),
    "strip2000": lambda: strip(2000),
    "heightfield10k": lambda: scene.heightfield_scene(71)[0],
    "nan_vertex": nan_scene,
}


@pytest.mark.parametrize("name", list(SCENES))
def test_build_lbvh_gives_a_valid_tree(name):
    tris = np.ascontiguousarray(SCENES[name]())
    nodes, perm = build_lbvh(tris)
    depth = check_tree(tris, nodes, perm, finite=name != "nan_vertex")
    n = tris.shape[0]
    assert depth <= 30 + max(1, int(np.ceil(np.log2(n)))) + 1
    if n <= LBVH_LEAF_TRIS:
        assert len(nodes) == 1 and nodes[0]["count"] == n  # the root is a leaf
    if name == "identical300":  # equal codes: the index bits split
        assert perm.tolist() == list(range(300))
    if name == "heightfield10k":
        assert n >= 10000


@pytest.mark.parametrize("leaf_tris", [1, 2, 8])
def test_other_leaf_sizes(leaf_tris):
    tris = scene.heightfield_scene(24)[0]
    nodes, perm = build_lbvh(tris, leaf_tris=leaf_tris)
    check_tree(tris, nodes, perm, leaf_tris=leaf_tris)


def test_tree_is_a_function_of_the_triangles_and_their_order():
    """Keys carry the CALLER'S index: equal codes are ordered by it.  Two calls with the same array give the same result byte for byte; a shuffled call gives
    the same leaf-order TRIANGLES and the same nodes once the shuffle is undone, provided no two triangles share a code — the heightfield at 10 bits per axis."""
    tris = scene.heightfield_scene(24)[0]
    assert len(set(codes(tris).tolist())) == tris.shape[0]
    nodes, perm = build_lbvh(tris)
    again = build_lbvh(tris.copy())
    assert nodes.tobytes() == again[0].tobytes() and np.array_equal(perm, again[1])
    shuffle = np.random.default_rng(5).permutation(tris.shape[0])
    nodes_s, perm_s = build_lbvh(tris[shuffle])
    assert np.array_equal(shuffle[perm_s], perm)  # the shuffle undone: the same caller's triangle in every leaf slot
    assert nodes_s.tobytes() == nodes.tobytes()
    # with equal codes the caller's order decides: 300 identical triangles stay in the order given, whatever it is
    same = np.repeat(tris[:1], 300, axis=0)
    same[:, 12] = np.arange(300) % 3
    _, p = build_lbvh(same[::-1])
    assert p.tolist() == list(range(300))
