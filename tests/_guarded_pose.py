"""The numpy statement of one GUARDED POSE UPDATE (include/rvpt_hip.h: RVPT_HIP_NODES_UPDATE_POSE_GUARDED) on a context whose tree a build form made, for
tests/test_guarded_pose_host.py and tests/test_guarded_pose.py: pose the listed parts from the rest pose, refit the paths above them, cost the tree, and past the
limit rebuild by the tree's builder from the posed triangles — while the rest pose stays what it was.  Built from scene.pose_parts, scene.refit_bvh(touched=),
scene.tree_cost and the three numpy builders.  Everything is in the CALLER'S order except what `perm` is applied to.  A plain module: no fixture, no GPU."""
from typing import NamedTuple, Optional

import numpy as np

from rvpt_amd import scene

LIMIT = 1.1
BUILDERS = {"lbvh": scene.build_lbvh, "ploc": scene.build_ploc, "sah": scene.build_sah}


class State(NamedTuple):
    """what a context holds, stated on the host: the tree (a numpy builder's layout) over current[perm], the permutation, the base cost, the rest pose and the
    triangles as they stand, both float32[n, 16] in the caller's order"""
    nodes: np.ndarray
    perm: np.ndarray
    base: float
    rest: np.ndarray
    current: np.ndarray


class Step(NamedTuple):
    state: State
    cost: float      # of the posed tree, the one the decision is taken by
    rebuilt: bool
    touched: np.ndarray  # the listed positions in the stored order of BEFORE the step


def built(tris, method) -> State:
    """the state after build_scene(tris, mats, method): no pose yet, so the rest pose is the triangles"""
    tris = np.ascontiguousarray(tris, dtype=np.float32)
    nodes, perm = BUILDERS[method](tris)[:2]
    return State(nodes, np.asarray(perm, dtype=np.int64), scene.tree_cost(nodes), tris, tris)


def listed_of(moves) -> np.ndarray:
    rec = scene.part_moves(moves)
    return np.concatenate([np.arange(int(r["first"]), int(r["first"]) + int(r["count"]), dtype=np.int64) for r in rec])


def permille_of(limit) -> int:
    """the limit as the count carries it: None or inf is 0 (report only), a factor is rounded to thousandths"""
    return 0 if limit is None or limit == np.inf else int(round(float(limit) * 1000.0))


def step(state: State, moves, limit: Optional[float], method: str) -> Step:
    """(nodes, perm, base, rest, current) + moves + a limit -> (nodes', perm', base', current', cost, rebuilt); rest' = rest, always"""
    posed = scene.pose_parts(state.rest, moves, current=state.current)
    inverse = np.empty(state.perm.shape[0], dtype=np.int64)
    inverse[state.perm] = np.arange(state.perm.shape[0])
    touched = inverse[listed_of(moves)]
    refit = scene.refit_bvh(state.nodes, posed[state.perm], touched=touched)
    cost = scene.tree_cost(refit)
    permille = permille_of(limit)
    if permille == 0 or not cost > permille / 1000.0 * state.base:  # the rule of the guarded update, in its arithmetic
        return Step(State(refit, state.perm, state.base, state.rest, posed), cost, False, touched)
    nodes, perm = BUILDERS[method](posed)[:2]
    return Step(State(nodes, np.asarray(perm, dtype=np.int64), scene.tree_cost(nodes), state.rest, posed), cost, True, touched)


# ---- the motions of the tests ----------------------------------------------------------------------------------------------------------------------------------

def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def about(centre, rot):
    """the 3x4 matrix of x -> R (x - c) + c"""
    c = np.asarray(centre, dtype=np.float64)
    return np.concatenate([rot, (c - rot @ c).reshape(3, 1)], axis=1)


def centroid(tris, first, count):
    return tris[first:first + count].reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64).mean(axis=0)


def extent_x(tris) -> float:
    return float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, 0]))


def part_of(n):
    """the part of the issue's table: a tenth of the mesh from a third of the way in, in the caller's order"""
    return n // 3, n // 10


def second_part_of(n):
    return 2 * n // 3, n // 20


def turned(tris, first, count, degrees):
    """the part rotated about its centroid, about an axis a little off the vertical"""
    return (first, count, about(centroid(tris, first, count), rotation((0.2, 1, 0.1), np.radians(degrees))))


def carried(tris, first, count):
    """the part carried half the scene's extent along x"""
    return (first, count, np.concatenate([np.eye(3), np.array([[0.5 * extent_x(tris)], [0.0], [0.0]])], axis=1))


def sequence(tris):
    """the four steps: the part turned by 2 degrees; the part carried; a second part turned by 3 degrees; the first part turned 2 degrees the other way beside an
    identity pose of the second — both from the rest pose, which is what fails if the rest pose was lost or mis-permuted by the rebuild of step two"""
    n = tris.shape[0]
    f, c = part_of(n)
    f2, c2 = second_part_of(n)
    return [[turned(tris, f, c, 2.0)],
            [carried(tris, f, c)],
            [turned(tris, f2, c2, 3.0)],
            [turned(tris, f, c, -2.0), (f2, c2, np.eye(3, 4))]]
