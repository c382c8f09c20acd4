"""The numpy statement of one GUARDED SKIN UPDATE (include/rvpt_hip.h: RVPT_HIP_NODES_UPDATE_SKIN_GUARDED) on a context whose tree a build form made, for
tests/test_guarded_skin_host.py and tests/test_guarded_skin.py: skin every vertex from the rest pose, refit every box, cost the tree, and past the limit rebuild
by the tree's builder from the skinned triangles — while the rest pose and the binding stay what they were.  Built from scene.skin_triangles, scene.refit_bvh
(every box), scene.tree_cost and the three numpy builders, as tests/_guarded_pose.py is built from its parts.  Everything is in the CALLER'S order except what
`perm` is applied to.  A plain module: no fixture, no GPU."""
from typing import NamedTuple, Optional

import numpy as np

import _skin
from _guarded_pose import BUILDERS, LIMIT, permille_of  # the same limit, the same builders and the same rounding of the limit as the guarded pose update's
from rvpt_amd import scene

N_BONES = 64  # the bones of the two sets below: enough of them that a block of four lies inside the model of the Cornell box (see carrying)


class State(NamedTuple):
    """what a context holds, stated on the host: the tree (a numpy builder's layout) over current[perm], the permutation, the base cost, the rest pose, the
    triangles as they stand (both float32[n, 16]) and the binding (VERTEX_SKIN_DTYPE[3 n]), the last three in the caller's order"""
    nodes: np.ndarray
    perm: np.ndarray
    base: float
    rest: np.ndarray
    current: np.ndarray
    skin: np.ndarray


class Step(NamedTuple):
    state: State
    cost: float      # of the skinned tree, the one the decision is taken by
    rebuilt: bool


def built(tris, method, skin) -> State:
    """the state after build_scene(tris, mats, method) and bind_skin(skin): nothing moved yet, so the rest pose is the triangles"""
    tris = np.ascontiguousarray(tris, dtype=np.float32)
    nodes, perm = BUILDERS[method](tris)[:2]
    return State(nodes, np.asarray(perm, dtype=np.int64), scene.tree_cost(nodes), tris, tris, scene.vertex_skins(skin))


def skinned_of(state: State, bones) -> np.ndarray:
    """every vertex from the rest pose; the mat_id rows as they stand, and the w lanes too (the rest pose's are the current ones: no form that keeps the rest
    pose writes them)"""
    out = scene.skin_triangles(state.rest, state.skin, bones)
    assert np.array_equal(out[:, [3, 7, 11]].view(np.uint32), state.current[:, [3, 7, 11]].view(np.uint32))
    out[:, 12:] = state.current[:, 12:]
    return out


def step(state: State, bones, limit: Optional[float], method: str) -> Step:
    """(nodes, perm, base, rest, current, skin) + bones + a limit -> (nodes', perm', base', current', cost, rebuilt); rest' = rest and skin' = skin, always"""
    skinned = skinned_of(state, bones)
    refit = scene.refit_bvh(state.nodes, skinned[state.perm])
    cost = scene.tree_cost(refit)
    permille = permille_of(limit)
    if permille == 0 or not cost > permille / 1000.0 * state.base:  # the rule of the guarded update, in its arithmetic
        return Step(State(refit, state.perm, state.base, state.rest, skinned, state.skin), cost, False)
    nodes, perm = BUILDERS[method](skinned)[:2]
    return Step(State(nodes, np.asarray(perm, dtype=np.int64), scene.tree_cost(nodes), state.rest, skinned, state.skin), cost, True)


# ---- the bones of the tests --------------------------------------------------------------------------------------------------------------------------------------

def _points(tris):
    return np.asarray(tris, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)


def weights(tris, k=N_BONES):
    """tests/_skin.py's weights: the four nearest of k centres along the scene's diagonal"""
    return _skin.weights(tris, k)


def gentle(tris, k=N_BONES, phase=0.0):
    """float32[k, 3, 4]: every bone a rotation of one to two degrees about the scene's centre, about an axis of its own"""
    p = _points(tris)
    centre = 0.5 * (p.min(axis=0) + p.max(axis=0))
    out = np.zeros((k, 3, 4), dtype=np.float32)
    for b in range(k):
        a = 0.9 * b + phase
        rot = _skin.rotation((np.sin(a) + 0.2, 1.0, np.cos(1.7 * a)), np.radians(1.5 + 0.5 * np.sin(2.3 * a + 1.0)))
        out[b, :, :3] = rot
        out[b, :, 3] = centre - rot @ centre
    return out


def carried_bones(k=N_BONES):
    """two blocks of k/16 consecutive bones, a quarter and three eighths of the way along the diagonal.  (Blocks, because a vertex blends its four nearest
    bones: carried and uncarried bones in turn would average out to one translation of everything.  There, because Cornell's model lies there and the bones
    the corners of its walls follow do not: the walls are twelve triangles whose boxes no motion makes worse, and the room must not grow around the model.)"""
    w = max(k // 16, 1)
    return [b for start in (k // 4, 3 * k // 8) for b in range(start, min(start + w, k))]


def axes_by_extent(tris):
    """the axes, largest extent first (equal extents in the order x, y, z)"""
    return [int(a) for a in np.argsort(-np.ptp(_points(tris), axis=0), kind="stable")]


def carrying(tris, k=N_BONES, axis=None, phase=0.4):
    """the gentle set of another phase with the bones of carried_bones translated by half the scene's largest extent along `axis` (default: the axis of the
    second largest extent): the triangles between a carried block and its neighbours stretch across the scene"""
    p = _points(tris)
    ext = np.ptp(p, axis=0)
    axis = axes_by_extent(tris)[1] if axis is None else axis
    out = gentle(tris, k, phase)
    for b in carried_bones(k):
        out[b, axis, 3] += np.float32(0.5 * ext.max())
    return out


def sequence(tris, k=N_BONES):
    """the four steps: gentle; carrying along the axis of the second largest extent; gentle with other angles; carrying along the axis of the largest extent —
    all from the rest pose, which is what fails if the rest pose was lost or mis-permuted by the rebuild of step two.  (Every skin update is absolute: step
    three needs the tree built on the carried pose to hold for the gentle one, step four needs it not to hold for a pose carried elsewhere.  The sets were
    tuned on the CPU until cornell_scene(2) and heightfield_scene(16) gave refit, rebuild, refit, rebuild under all three builders; the limit was not.)"""
    order = axes_by_extent(tris)
    return [gentle(tris, k), carrying(tris, k, order[1], 0.4), gentle(tris, k, 2.0), carrying(tris, k, order[0], 1.0)]


# ---- what the GPU tests call with a limit, restated here so that tests/test_guarded_skin_host.py can hold every ratio away from its limit ------------------------

SEQUENCE_SCENES = ("terrain16", "cornell2", "default")
METHODS = ("lbvh", "ploc", "sah")
SHAPE_BONES = (1, 3, 1024)


def tris_of(name):
    return {"terrain16": lambda: scene.heightfield_scene(16), "cornell2": lambda: scene.cornell_scene(2), "default": scene.default_scene,
            "terrain184": lambda: scene.heightfield_scene(184)}[name]()


def shape_steps(tris, k):
    """the two calls of the shapes test: tests/_skin.py's small motions, then the carrying set (with one bone or three nothing is carried far: a refit)"""
    return [_skin.bones(tris, k), carrying(tris, k)]


def big_case():
    """tests/test_skin_update.py's 67 712 triangles with 1024 bones and random influences; the carrying set tears every triangle apart"""
    tris, mats = scene.heightfield_scene(184)
    tris = np.ascontiguousarray(tris)
    n = tris.shape[0]
    rng = np.random.RandomState(7)
    rec = np.zeros(3 * n, dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"] = rng.randint(0, 1024, size=(3 * n, 4))
    w = rng.uniform(0.1, 1.0, size=(3 * n, 4))
    rec["weight"] = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    rec["bone"][0, 0], rec["bone"][-1, 3] = 1023, 1023
    return tris, np.ascontiguousarray(mats), rec, carrying(tris, 1024)


def cpp_selftest_case():
    """rvpt_amd/host/host_selftest_skin_guard.cpp's --gpu leg restated: terrain(12) (288 triangles over [-2, 2] x [2, 6], heights from its formula in float32),
    bands_of (one bone per vertex, four bands of width 1 along x), and the two bone sets it sends under a limit of 1.1, bone_of's arithmetic in float32.
    Returns (tris, skin, [gentle, carrying]).  (numpy's float32 sine and the C library's may differ in the last place: the ratios lie percents from the limit.)"""
    cells = 12
    f = np.float32

    def p(i, j):
        x, z = f(-2.0) + f(4.0) * f(i) / f(cells), f(2.0) + f(4.0) * f(j) / f(cells)
        return [x, f(-1.0) + f(0.2) * np.sin(f(1.7) * x) * np.cos(f(1.3) * z), z]
    pos = []
    for j in range(cells):
        for i in range(cells):
            pos.append([p(i, j), p(i + 1, j), p(i + 1, j + 1)])
            pos.append([p(i, j), p(i + 1, j + 1), p(i, j + 1)])
    tris = scene.make_triangles(np.array(pos, dtype=np.float32), 0)
    x = tris.reshape(-1, 4, 4)[:, :3, 0].reshape(-1)
    rec = np.zeros(x.shape[0], dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"][:, 0] = np.clip((x + f(2.0)).astype(np.int64), 0, 3)
    rec["weight"][:, 0] = 1.0

    def bone_of(degrees, tz):
        a = degrees * 3.14159265358979323846 / 180.0
        c, s_, cx, cz = f(np.cos(a)), f(np.sin(a)), f(0.0), f(4.0)
        return [c, 0, s_, cx - c * cx - s_ * cz, 0, 1, 0, 0, -s_, 0, c, cz + s_ * cx - c * cz + f(tz)]
    gentle_set = np.array([bone_of(1.0, 0.0), bone_of(-1.5, 0.0), bone_of(2.0, 0.0), bone_of(-1.0, 0.0)], dtype=np.float32)
    carrying_set = gentle_set.copy()
    carrying_set[1] = np.array(bone_of(-1.5, 2.0), dtype=np.float32)
    return tris, rec, [gentle_set, carrying_set]


def mirror_steps(tris):
    """the three calls of the renderer mirror's test under the limit: gentle, carrying, and the SAME gentle set again on the tree built at the carried pose"""
    return [gentle(tris), carrying(tris), gentle(tris)]


def gpu_ratios():
    """(what, ratio, limit) of every call the GPU tests make with a limit — the same inputs through the same functions"""
    for name in SEQUENCE_SCENES:
        tris = np.ascontiguousarray(tris_of(name)[0])
        for method in METHODS:
            st = built(tris, method, weights(tris))
            for j, bones in enumerate(sequence(tris)):
                r = step(st, bones, LIMIT, method)
                yield f"{name} {method} step {j + 1}", r.cost / st.base, LIMIT
                st = r.state
    tris = np.ascontiguousarray(tris_of("default")[0])
    for k in SHAPE_BONES:
        for method in METHODS:
            st = built(tris, method, weights(tris, k))
            for j, bones in enumerate(shape_steps(tris, k)):
                r = step(st, bones, LIMIT, method)
                yield f"default {k} bones {method} call {j + 1}", r.cost / st.base, LIMIT
                st = r.state
    tris, _, rec, bones = big_case()
    st = built(tris, "lbvh", rec)
    yield "terrain184 lbvh", step(st, bones, LIMIT, "lbvh").cost / st.base, LIMIT
    tris = np.ascontiguousarray(tris_of("terrain16")[0])
    st = built(tris, "sah", weights(tris))
    for j, bones in enumerate(mirror_steps(tris)):
        r = step(st, bones, LIMIT, "sah")
        yield f"the renderer mirror, terrain16 sah call {j + 1}", r.cost / st.base, LIMIT
        st = r.state
    tris, rec, sets = cpp_selftest_case()
    st = built(tris, "sah", rec)
    for what, bones in zip(("gentle", "carrying"), sets):
        r = step(st, bones, LIMIT, "sah")
        yield f"host_selftest_skin_guard --gpu, {what}", r.cost / st.base, LIMIT
        st = r.state
