"""scene.tree_cost: the numpy statement of the number the guarded update of rvpt_hip_upload_scene reports (include/rvpt_hip.h) — the SAH cost of a tree — against tests/test_ploc_host.py's sah_cost on the three builders' trees, and on the trees whose cost can be said by hand."""
import numpy as np
import pytest

from rvpt_amd import scene
from rvpt_amd.scene import NODE_DTYPE, build_lbvh, build_ploc, build_sah, refit_bvh, tree_cost
from test_ploc_host import sah_cost

SCENES = {"default": scene.default_scene, "cornell": scene.cornell_scene, "terrain16": lambda: scene.heightfield_scene(16)}
BUILDERS = {"lbvh": build_lbvh, "ploc": build_ploc, "sah": build_sah}
_TREES = {}


def tree_of(name, method):
    """(tris, nodes as NODE_DTYPE records, perm) — built once, shared and left unchanged"""
    if (name, method) not in _TREES:
        tris = np.ascontiguousarray(SCENES[name]()[0])
        nodes, perm = BUILDERS[method](tris)[:2]
        _TREES[name, method] = (tris, np.ascontiguousarray(nodes).view(NODE_DTYPE).reshape(-1), perm)
    return _TREES[name, method]


@pytest.mark.parametrize("method", list(BUILDERS))
@pytest.mark.parametrize("name", list(SCENES))
def test_tree_cost_is_sah_cost(name, method):
    _, nodes, _ = tree_of(name, method)
    got, want = tree_cost(nodes), sah_cost(nodes)
    print(f"{name} {method}: {nodes.shape[0]} nodes, tree_cost {got!r}, sah_cost {want!r}, relative difference {abs(got - want) / want:.3e}")
    assert got > 1.0
    assert abs(got - want) <= 1e-12 * want


@pytest.mark.parametrize("method", list(BUILDERS))
@pytest.mark.parametrize("name", list(SCENES))
def test_refit_with_the_same_triangles_keeps_the_cost(name, method):
    """the builders' boxes are tight: refit_bvh gives them back, and the cost with them"""
    tris, nodes, perm = tree_of(name, method)
    assert tree_cost(refit_bvh(nodes, tris[perm])) == tree_cost(nodes)


def test_raw_words_and_records_are_the_same_tree():
    _, nodes, _ = tree_of("default", "sah")
    assert tree_cost(nodes.view(np.uint32).reshape(-1, 8)) == tree_cost(nodes)


@pytest.mark.parametrize("count", [1, 2, 7])
def test_a_one_leaf_tree_costs_its_triangle_count(count):
    nodes = np.zeros(1, dtype=NODE_DTYPE)
    nodes[0] = (0, count, (-1.0, 2.0, 0.5, 0.75, -3.0, 4.0))
    assert tree_cost(nodes) == float(count)


def test_a_flat_root_costs_nothing():
    """half-area 0: a point, or a box with extent on one axis only; a box flat on one axis has an area and a cost"""
    nodes = np.zeros(3, dtype=NODE_DTYPE)
    nodes[0] = (1, 0, (1.0, 1.0, 2.0, 2.0, 3.0, 3.0))
    nodes[1] = (0, 1, (1.0, 1.0, 2.0, 2.0, 3.0, 3.0))
    nodes[2] = (1, 1, (1.0, 1.0, 2.0, 2.0, 3.0, 3.0))
    assert tree_cost(nodes) == 0.0
    nodes["bounds"][:, 1] = 5.0  # extent on x alone
    assert tree_cost(nodes) == 0.0
    nodes["bounds"][:, 3] = 4.0  # x and y: flat on z, area 4 * 2
    assert tree_cost(nodes) == 3.0
    assert tree_cost(np.zeros(0, dtype=NODE_DTYPE)) == 0.0


def test_two_leaves_by_hand_and_strays_left_out():
    """root 2 x 2 x 2 (half-area 12) over a 1 x 2 x 2 leaf of three triangles (half-area 8) and a 1 x 1 x 1 leaf of one (half-area 3): (12 + 24 + 3) / 12; a
    fourth node the root does not reach changes nothing"""
    nodes = np.zeros(4, dtype=NODE_DTYPE)
    nodes[0] = (1, 0, (0, 2, 0, 2, 0, 2))
    nodes[1] = (0, 3, (0, 1, 0, 2, 0, 2))
    nodes[2] = (3, 1, (1, 2, 1, 2, 1, 2))
    nodes[3] = (0, 9, (-100, 100, -100, 100, -100, 100))
    assert tree_cost(nodes) == 39.0 / 12.0
    assert tree_cost(nodes[:3]) == 39.0 / 12.0


def test_the_extents_are_taken_in_double():
    """hi - lo from the float32 bounds widened to double, as sah_cost and the device take it: 1 - 1e-8 is 1 in float32 and short of 1 in double"""
    lo, hi = np.float32(1e-8), np.float32(1.0)
    assert np.float32(hi - lo) == np.float32(1.0)  # a float32 subtraction would round the small bound away
    nodes = np.zeros(3, dtype=NODE_DTYPE)
    nodes[0] = (1, 0, (0, 1, 0, 1, 0, 1))
    nodes[1] = (0, 1, (lo, hi, lo, hi, lo, hi))
    nodes[2] = (1, 1, (0, 1, 0, 1, 0, 1))
    e = 1.0 - float(lo)
    assert tree_cost(nodes) == (3.0 + 3.0 * e * e + 3.0) / 3.0 < 3.0
