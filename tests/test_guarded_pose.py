"""The guarded pose update on the GPU: rvpt_hip_upload_scene's RVPT_HIP_NODES_UPDATE_POSE_GUARDED form (Context.pose_parts(rebuild_above=)) poses parts from the
rest pose, costs the stored tree and, past a limit, rebuilds it by the builder that made it — and the rest pose follows the triangles through the rebuild.  The
reported numbers against the numpy statement of one step (tests/_guarded_pose.py) at 1e-9 relative; everything else bit for bit: images, segment counts and
launches against fresh contexts and the CPU oracle, and in the laboratory build the triangles, the nodes, the wide form, the permutation and the rest pose
against the statement after every step."""
import ctypes
import math

import numpy as np
import pytest

import _device_state as ds
import _guarded_pose as gp
import _ray_query as rq
from test_device_build import camera_for, native  # noqa: F401  (native: the module's fixture)
from test_device_state import same_state
from test_gpu_parity import _loosen_boxes, oracle_frames
from test_refit import bits, flags_of, render

pytestmark = pytest.mark.gpu

W, H = 64, 48
REL = 1e-9  # double summation over n <= 2^21 terms in any order errs by at most n * 2^-53 = 2.3e-10 relative
_SCENES, _BUILT = {}, {}


def scene_of(name):
    """(tris in the generator's order, mats, camera) — made once, shared and left unchanged"""
    if name not in _SCENES:
        from rvpt_amd import scene
        if name == "two":
            tris, mats = scene.default_scene()
            tris = tris[100:102]
        else:
            tris, mats = {"terrain16": lambda: scene.heightfield_scene(16), "terrain64": lambda: scene.heightfield_scene(64), "cornell2": lambda: scene.cornell_scene(2),
                          "default": scene.default_scene}[name]()
        tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
        tris.setflags(write=False)
        cam = camera_for({"cornell2": "cornell", "two": "default"}.get(name, name), W, H)
        _SCENES[name] = (tris, mats, cam)
    return _SCENES[name]


def built_of(name, method):
    if (name, method) not in _BUILT:
        _BUILT[name, method] = gp.built(scene_of(name)[0], method)
    return _BUILT[name, method]


def close(a, b):
    return abs(a - b) <= REL * abs(b)


def said(ctx):
    return (ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode()


def raw_pose(native, ctx, rec, count, k=None, tris=None, mats=None, offset=0):
    """the C call itself: (return code, message); rec: PART_MOVE_DTYPE records or None; count: the n_nodes argument"""
    keep = None if rec is None else np.ascontiguousarray(rec)
    ptr = None if keep is None else ctypes.c_void_p(keep.ctypes.data + offset)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=np.float32)
    m = None if mats is None else np.ascontiguousarray(mats, dtype=np.float32)
    rc = ctx._L.rvpt_hip_upload_scene(ctx._h, ptr, count, None if t is None else t.ctypes.data_as(ctypes.c_void_p), (0 if keep is None else keep.shape[0]) if k is None else k,
                                      None if m is None else m.ctypes.data_as(ctypes.c_void_p), 0 if m is None else m.shape[0])
    return rc, said(ctx)


def usable(ratio, limit):
    """the device adds in another order than numpy: a case decides alike where its ratio is a thousandth or more away from the limit"""
    if abs(ratio / limit - 1.0) < 1e-3:
        pytest.fail(f"misconfigured case: the ratio {ratio:.6f} lies within a thousandth of the limit {limit}")


def check_against_statement(state, before, st, r, what):
    """the laboratory read-back `state` after a step against the statement: r = gp.step(st, ...); before: the read-back in front of the step"""
    new = r.state
    dev = ds.shifted_layout(new.nodes)
    assert ds.same_nodes(state["nodes"], dev), (what, "d_nodes", ds.first_difference(state["nodes"], dev))
    assert ds.same_bytes(state["perm"], new.perm.astype(np.uint32)), (what, "d_perm")
    assert ds.same_bytes(state["tris"], new.current[new.perm]), (what, "d_tris", ds.first_difference(state["tris"], new.current[new.perm]))
    assert ds.same_bytes(state["rest"], new.rest[new.perm][:, :12]), (what, "REST is the old rest pose in the new stored order", ds.first_difference(state["rest"], new.rest[new.perm][:, :12]))
    assert state["have_cost"] and state["have_perm"], what
    if r.rebuilt:
        assert close(state["base_cost"], new.base), (what, state["base_cost"], new.base)
    else:
        assert state["base_cost"] == before["base_cost"] and close(state["base_cost"], st.base), what
        want_wide = ds.regathered(before["wide"], before["wide_map"], dev)
        assert ds.same_bytes(state["wide"], want_wide), (what, "d_wide", ds.first_difference(state["wide"], want_wide))
        assert ds.same_bytes(state["wide_map"], before["wide_map"]) and ds.same_bytes(state["refit_levels"], before["refit_levels"]), what
    ds.check_wide_map(state, what)


def guarded_step(native, ctx, st, moves, limit, method, what, before=None):
    """one call and its statement: the report against the statement's numbers and decision, and the read-back where the context is a laboratory one"""
    r = gp.step(st, moves, limit, method)
    if gp.permille_of(limit):
        usable(r.cost / st.base, gp.permille_of(limit) / 1000.0)
    if before is None and ctx.lab:
        before = ctx.scene_state()
    rep = ctx.pose_parts(moves, rebuild_above=limit)
    print(f"{what}: device {said(ctx)}; numpy cost {r.cost!r}, base {st.base!r}, ratio {r.cost / st.base:.6f}, rebuilt {r.rebuilt}")
    assert close(rep.cost, r.cost), (what, rep.cost, r.cost)
    assert close(rep.base_cost, st.base), (what, rep.base_cost, st.base)
    assert rep.rebuilt == r.rebuilt and rep.tree == (method if r.rebuilt else None), (what, rep)
    state = None
    if ctx.lab:
        state = ctx.scene_state()
        check_against_statement(state, before, st, r, what)
    return r, rep, state


# ---- the count is a form ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_count_is_a_form_of_the_call(native, method):
    """until this form existed the call answered "NULL scene array" """
    from rvpt_amd import scene
    tris, mats, _ = scene_of("default")
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        rc, msg = raw_pose(native, ctx, scene.part_moves([(0, 5, np.eye(3, 4))]), native.nodes_update_pose_guarded(0))
        assert rc == 0, msg
        assert msg.startswith("guarded pose update: cost ") and msg.endswith(", limit 0 permille: refitted")
    finally:
        ctx.close()


# ---- numbers --------------------------------------------------------------------------------------------------------------------------------------------------

NUMBER_CASES = [("terrain16", "lbvh"), ("terrain16", "ploc"), ("terrain16", "sah"), ("terrain64", "lbvh"), ("two", "lbvh")]


@pytest.mark.parametrize("name,method", NUMBER_CASES, ids=[f"{n}-{m}" for n, m in NUMBER_CASES])
def test_the_reported_cost_is_tree_cost_of_the_posed_tree(native, name, method):
    tris, mats, _ = scene_of(name)
    st = built_of(name, method)
    n = tris.shape[0]
    if (name, method) == ("terrain16", "lbvh"):
        assert len(st.nodes) > 256  # more than one partial
    if name == "terrain64":
        assert len(st.nodes) > 32 * 256
    first, count = (0, 1) if name == "two" else gp.part_of(n)
    moves = [gp.turned(tris, first, count, 2.0)]
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        r, rep, _ = guarded_step(native, ctx, st, moves, math.inf, method, f"{name} {method}")
        first_said = said(ctx)
        assert rep.ratio == rep.cost / rep.base_cost
        assert first_said == f"guarded pose update: cost {rep.cost:.17g}, base cost {rep.base_cost:.17g}, limit 0 permille: refitted"  # %.17g: the doubles come back as they were
        ctx.pose_parts(moves, rebuild_above=math.inf)
        assert said(ctx) == first_said, "the same tree must give the same 64 bits on every run"
        if name == "two":  # one node: the cost is the leaf's count whatever the vertices do, and nothing ever rebuilds
            assert len(st.nodes) == 1 and rep.cost == rep.base_cost == 2.0
            far = ctx.pose_parts([gp.carried(tris, 0, 1)], rebuild_above=1.0)
            assert far.cost == 2.0 and not far.rebuilt
    finally:
        ctx.close()


# ---- the sequence -----------------------------------------------------------------------------------------------------------------------------------------------

def fresh_of(native, fl, upload, cam, batch):
    """(image, (segments, samples), launch_info()[:3], read-back) of a fresh laboratory context after upload(ctx)"""
    ctx = native.Context(W, H, 0, 0, 1, fl, lab=True)
    try:
        upload(ctx)
        state = ctx.scene_state()
        img = render(ctx, cam, 2, batch=batch)
        return img, ctx.stats(), ctx.launch_info()[:3], state
    finally:
        ctx.close()


def run_sequence(native, oracle, name, method, traversal, batch, path=None):
    tris, mats, cam = scene_of(name)
    st = built_of(name, method)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS)
    ctx = native.Context(W, H, 0, 0, 1, fl, lab=True)
    decisions = []
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        before = ctx.scene_state()
        still = render(ctx, cam, 2, batch=batch)
        seen, info = ctx.stats(), ctx.launch_info()[:3]
        if path is not None:
            assert info[2] == path
        for j, moves in enumerate(gp.sequence(tris)):
            what = f"{name} {method} {traversal} step {j + 1}"
            r, rep, state = guarded_step(native, ctx, st, moves, gp.LIMIT, method, what, before=before)
            decisions.append(r.rebuilt)
            got = render(ctx, cam, 2, batch=batch)
            now = ctx.stats()
            new = r.state
            stored = new.current[new.perm]
            if r.rebuilt:  # the context holds what a fresh build of the posed triangles holds, the rest pose apart
                want, want_stats, want_info, want_state = fresh_of(native, fl, lambda c: c.build_scene(new.current, mats, method=method), cam, batch)
                same_state(state, want_state, but=("rest",))
                assert ctx.launch_info()[:3] == want_info, (what, ctx.launch_info()[:3], want_info)
            else:  # ... or what an upload of the statement's refit holds
                want, want_stats, want_info, _ = fresh_of(native, fl, lambda c: c.upload_scene(new.nodes, stored, mats), cam, batch)
                # the kernel path is the fresh upload's; the LDS bytes follow the grouping of the wide form, which a refit keeps from the build and a fresh upload of
                # the moved tree may make anew (include/rvpt_hip.h: POSE UPDATE), so they stay the context's own
                assert ctx.launch_info()[2] == want_info[2] == info[2] and ctx.launch_info()[1] == info[1], (what, ctx.launch_info()[:3], want_info, info)
            ref, seg = oracle_frames(oracle, (stored, mats, new.nodes), cam, W, H, traversal, [0, 1])
            assert np.array_equal(bits(got), bits(want)), f"{what}: the image of the fresh context"
            assert np.array_equal(bits(got), bits(ref[1])), f"{what}: the oracle's image on the statement's tree"
            assert (now[0] - seen[0], now[1] - seen[1]) == want_stats and want_stats[0] == seg, (what, now, seen, want_stats, seg)
            assert not np.array_equal(bits(got), bits(still)), f"{what}: the geometry did not move"
            st, before, seen, info, still = new, state, now, ctx.launch_info()[:3], got
    finally:
        ctx.close()
    return decisions


@pytest.mark.parametrize("traversal", ["bvh", "bvh_ordered"])
@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_sequence_on_the_terrain(native, oracle, method, traversal):
    """refit, rebuild, refit, rebuild — and step four poses from the rest pose through the permutation step two made"""
    assert run_sequence(native, oracle, "terrain16", method, traversal, False) == [False, True, False, True]


@pytest.mark.parametrize("traversal", ["bvh", "bvh_ordered"])
@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_sequence_on_cornell(native, oracle, method, traversal):
    """2300 triangles, no multiple of 64 or 256; the fourth decision lies near the limit and is the statement's (tests/test_guarded_pose_host.py)"""
    assert run_sequence(native, oracle, "cornell2", method, traversal, False)[:3] == [False, True, False]


def test_the_sequence_on_the_hbm_resident_wide_walk(native, oracle, monkeypatch):
    monkeypatch.setenv("RVPT_HIP_BVH_NO_RESIDENT", "1")
    assert run_sequence(native, oracle, "terrain16", "sah", "bvh", False, path=10) == [False, True, False, True]


def test_the_sequence_in_batched_launches(native, oracle):
    assert run_sequence(native, oracle, "terrain16", "ploc", "bvh", True) == [False, True, False, True]


# ---- afterwards -------------------------------------------------------------------------------------------------------------------------------------------------

def test_after_a_rebuild_every_form_answers_as_on_the_fresh_build(native):
    from rvpt_amd import scene
    name, method = "terrain16", "sah"
    tris, mats, cam = scene_of(name)
    n = tris.shape[0]
    first, count = gp.part_of(n)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl, lab=True), native.Context(W, H, 0, 0, 1, fl, lab=True)

    def alike(what, but=("rest",)):
        sa, sb = a.scene_state(), b.scene_state()
        same_state(sa, sb, but=but)
        assert np.array_equal(bits(render(a, cam, 2)), bits(render(b, cam, 2))), what
        return sa, sb

    try:
        assert a.build_scene(tris, mats, method=method) == method
        r, _, _ = guarded_step(native, a, built_of(name, method), [gp.carried(tris, first, count)], gp.LIMIT, method, "carried")
        assert r.rebuilt
        current = r.state.current
        assert b.build_scene(current, mats, method=method) == method
        alike("rebuilt")
        # ray and path queries: prim numbers the caller's order on both
        records = rq.poisoned(rq.base_rays(current, 11, counts=(80, 80, 50, 40, 30, 20)))
        ga, gb = a.trace_rays_into(records.copy()), b.trace_rays_into(records.copy())
        assert rq.same_bytes(ga, gb), rq.first_difference(ga, gb)
        hit = ga["prim"] != rq.NO_PRIM
        assert int(hit.sum()) > 50 and int(ga["prim"][hit].max()) < n
        rng = np.random.RandomState(3)
        org = np.tile(np.array([0.0, 2.5, -5.0], np.float32), (256, 1))
        dirs = rng.normal(size=(256, 3)).astype(np.float32)
        dirs[:, 2], dirs[:, 1] = np.abs(dirs[:, 2]) + 1.0, -np.abs(dirs[:, 1]) - 0.3
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True).astype(np.float32)
        seeds = rng.randint(0, 2 ** 31, 256).astype(np.uint32)
        pa, pb = a.trace_paths(org, dirs, seeds, 6), b.trace_paths(org, dirs, seeds, 6)
        assert pa.tobytes() == pb.tobytes() and int(pa["segments"].sum()) > 256
        # a plain pose of another part: from the rest pose of before the rebuild; on the fresh build the same vertices by a sparse update of the part's rows
        f2, c2 = gp.second_part_of(n)
        moves = [gp.turned(tris, f2, c2, 3.0), gp.turned(tris, first, count, 1.0)]
        posed = scene.pose_parts(tris, moves, current=current)
        assert a.pose_parts(moves) is None and said(a) == ""
        idx = gp.listed_of(moves)
        b.update_triangles(posed[idx], indices=idx)
        sa, _ = alike("a plain pose after the rebuild")
        assert ds.same_bytes(sa["tris"], posed[sa["perm"].astype(np.int64)]) and ds.same_bytes(sa["rest"], tris[sa["perm"].astype(np.int64)][:, :12])
        # a sparse update, numbered in the caller's order: the rest pose goes, as after every other form
        rows = scene.wobble(posed, 0.7, 0.05)[10:40]
        a.update_triangles(rows, indices=np.arange(10, 40))
        b.update_triangles(rows, indices=np.arange(10, 40))
        sa, _ = alike("a sparse update after the rebuild", but=())
        assert sa["rest"].size == 0
        # a plain update in the caller's order
        moved = scene.wobble(tris, 1.9, 0.05)
        a.update_triangles(moved)
        b.update_triangles(moved)
        alike("a plain update after the rebuild", but=())
    finally:
        a.close()
        b.close()


def test_plain_and_guarded_poses_share_one_rest_pose(native):
    from rvpt_amd import scene
    name, method = "terrain16", "ploc"
    tris, mats, _ = scene_of(name)
    n = tris.shape[0]
    first, count = gp.part_of(n)
    f2, c2 = gp.second_part_of(n)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        st = built_of(name, method)
        # plain, then guarded: the guarded one finds the snapshot the plain one took
        A = [gp.turned(tris, first, count, 5.0)]
        assert ctx.pose_parts(A) is None
        plain = gp.step(st, A, None, method)
        r, _, _ = guarded_step(native, ctx, plain.state, [gp.turned(tris, f2, c2, 3.0)], math.inf, method, "guarded after plain")
        # guarded with a rebuild, then plain: the plain one poses from the rest pose the rebuild carried along
        r, _, s1 = guarded_step(native, ctx, r.state, [gp.carried(tris, first, count)], gp.LIMIT, method, "carried")
        assert r.rebuilt
        back = [(first, count, np.eye(3, 4)), (f2, c2, np.eye(3, 4))]
        assert ctx.pose_parts(back) is None
        s2 = ctx.scene_state(["tris", "rest", "perm"])
        perm = r.state.perm
        assert ds.same_bytes(s2["perm"], s1["perm"]) and ds.same_bytes(s2["rest"], tris[perm][:, :12])
        assert ds.same_bytes(s2["tris"], scene.pose_parts(tris, back)[perm]) and ds.same_bytes(s2["tris"][:, :12], tris[perm][:, :12])  # (no coordinate here is -0)
    finally:
        ctx.close()


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------------------------

def shape_moves(shape, tris):
    from rvpt_amd import native as nat, scene
    n = tris.shape[0]
    if shape == "one_triangle":
        return [scene.part_move(n // 2, 1, translation=(0.3, 0.4, -0.2))]
    if shape == "whole_scene":  # flattened to a twentieth of its height: the cost is relative to the root's box, which a rigid motion of everything carries along
        return [(0, n, np.diag([1.0, 0.05, 1.0]) @ np.eye(3, 4))]
    assert shape == "every_triangle_a_part"
    out = np.zeros(n, dtype=nat.PART_MOVE_DTYPE)
    out["first"], out["count"] = np.arange(n), 1
    m = np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1))
    m[:, :, 3] = 0.3 * np.sin(np.arange(n)[:, None] * np.array([0.31, 0.17, 0.23]) + np.array([0.0, 1.0, 2.0]))
    out["m"] = m.reshape(n, 12)
    return out


# scene, list, limit, and whether the case is there for its rebuild (in numpy the flattened Cornell box costs 1.147 / 1.061 / 1.159 of its base: limit 1.02)
SHAPES = [("default", "one_triangle", gp.LIMIT, False), ("default", "every_triangle_a_part", gp.LIMIT, True), ("cornell2", "whole_scene", 1.02, True),
          ("cornell2", "one_triangle", gp.LIMIT, False)]


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
@pytest.mark.parametrize("name,shape,limit,rebuilds", SHAPES, ids=[f"{n}-{s}" for n, s, _, _ in SHAPES])
def test_shapes_of_the_list(native, name, shape, limit, rebuilds, method):
    """143 and 2300 triangles, no multiple of 64 or 256; the decision is the statement's, which must take the one the case is there for"""
    tris, mats, cam = scene_of(name)
    moves = shape_moves(shape, tris)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(W, H, 0, 0, 1, fl, lab=True)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        r, _, state = guarded_step(native, ctx, built_of(name, method), moves, limit, method, f"{name} {shape} {method}")
        assert r.rebuilt == rebuilds
        got = render(ctx, cam, 2)
        new = r.state
        if r.rebuilt:
            want, _, want_info, want_state = fresh_of(native, fl, lambda c: c.build_scene(new.current, mats, method=method), cam, False)
            same_state(state, want_state, but=("rest",))
            assert ctx.launch_info()[:3] == want_info
        else:
            want, _, _, _ = fresh_of(native, fl, lambda c: c.upload_scene(new.nodes, new.current[new.perm], mats), cam, False)
        assert np.array_equal(bits(got), bits(want))
        # and a pose from the rest pose afterwards, whatever was decided
        r2, _, _ = guarded_step(native, ctx, new, [gp.turned(tris, 3, 40, 4.0)], math.inf, method, f"{name} {shape} {method}, then a part turned")
    finally:
        ctx.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_scene_and_the_rest_pose_untouched(native):
    import torch
    from rvpt_amd import scene
    tris, mats, cam = scene_of("default")
    n = tris.shape[0]
    eye = np.eye(3, 4)
    ok = scene.part_moves([(0, 5, eye), (10, 5, eye), (20, 5, eye), (30, 5, eye)])
    count = native.nodes_update_pose_guarded(1100)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        rc, msg = raw_pose(native, ctx, ok, count)
        assert rc == native.ERR_INVALID and "pose update before any full upload_scene" in msg
        assert ctx.build_scene(tris, mats, method="sah") == "sah"
        ctx.pose_parts([gp.turned(tris, 0, 63, 20.0)], rebuild_above=math.inf)  # so that there is a rest pose to leave untouched
        img = render(ctx, cam, 2)
        s0 = ctx.scene_state()
        assert s0["rest"].shape == (n, 12)

        def untouched(what):
            same_state(ctx.scene_state(), s0)
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img)), what

        many = scene.part_moves([(j, 1, eye) for j in range(n)] + [(0, 1, eye)])
        count0, reserved, past, wraps = ok.copy(), ok.copy(), ok.copy(), ok.copy()
        count0["count"][1] = 0
        count0["first"][3] = n  # (position 3 offends too: position 1 is named)
        reserved["reserved"][2, 1] = 7
        past["first"][1], past["count"][1] = n - 2, 3
        past["first"][3] = n + 5
        wraps["first"][2], wraps["count"][2] = 0xFFFFFFFF, 2  # first + count wraps to 1
        overlap = scene.part_moves([(50, 10, eye), (0, 5, eye), (3, 4, eye), (55, 2, eye), (100, 1, eye)])
        nested = scene.part_moves([(100, 1, eye), (40, 3, eye), (0, 90, eye), (41, 1, eye)])
        cases = [((ok, count, 0), "pose update without parts"),  # every refusal of the pose form, in its words, reached through the new count
                 ((many, count), f"pose update with {n + 1} parts, the uploaded scene has {n} triangles"),
                 ((None, count, 4), "pose update without a list"),
                 ((np.concatenate([ok, ok]), count, 4, None, None, 2), "not 4-byte aligned"),
                 ((ok, count, None, tris[:4]), "takes no triangles"),
                 ((ok, count, None, None, mats), "takes no materials"),
                 ((count0, count), "moves[1] has a count of 0"),
                 ((reserved, count), "moves[2] has the reserved words 0, 7"),
                 ((past, count), f"moves[1] = [{n - 2}, {n - 2} + 3) is outside the {n} stored triangles"),
                 ((wraps, count), f"moves[2] = [4294967295, 4294967295 + 2) is outside the {n} stored triangles"),
                 ((overlap, count), "moves[0] = [50, 50 + 10) and moves[3] = [55, 55 + 2) share triangle 55"),
                 ((nested, count), "moves[1] = [40, 40 + 3) and moves[2] = [0, 0 + 90) share triangle 40")]
        for permille in (1, 999, 65536):  # ... and the one of the band
            cases.append(((ok, native.nodes_update_pose_guarded(permille)), f"guarded pose update: the limit is 0 (report only) or 1000 .. 65535 permille, got {permille}"))
        for args, what in cases:
            rc, msg = raw_pose(native, ctx, *args)
            assert rc == native.ERR_INVALID and what in msg, (what, rc, msg)
            untouched(what)
        dev = torch.from_numpy(ok.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        rc = ctx._L.rvpt_hip_upload_scene(ctx._h, ctypes.c_void_p(dev.data_ptr()), count, None, ok.shape[0], None, 0)
        assert rc == native.ERR_INVALID and "device memory" in said(ctx)
        untouched("device list")
        for bad in (0.5, float("nan"), 70, -1):
            with pytest.raises(native.NativeError, match="rebuild_above"):
                ctx.pose_parts(ok, rebuild_above=bad)
        untouched("the wrapper's refusals")
        for permille in (1000, 65535):  # the band's ends are forms of the call
            rc, msg = raw_pose(native, ctx, ok, native.nodes_update_pose_guarded(permille))
            assert rc == 0 and f"limit {permille} permille: " in msg, msg
    finally:
        ctx.close()


def test_after_an_ordinary_upload_a_limit_is_refused_and_a_report_is_legal(native):
    """the tree is the caller's, loose boxes included: report only gives the cost of the partly loose tree"""
    from rvpt_amd import scene
    tris, mats, cam = scene_of("default")
    st = built_of("default", "sah")
    stored = tris[st.perm]
    loose = _loosen_boxes(st.nodes, 4)
    moves = [gp.turned(stored, 20, 40, 15.0)]  # (after an ordinary upload the ranges are in the leaf order of that upload)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(loose, stored, mats)
        img = render(ctx, cam, 2)
        s0 = ctx.scene_state()
        for with_rest in (False, True):
            with pytest.raises(native.NativeError, match="guarded pose update with a limit after an ordinary upload_scene.*no builder") as e:
                ctx.pose_parts(moves, rebuild_above=gp.LIMIT)
            assert e.value.code == native.ERR_INVALID
            same_state(ctx.scene_state(), s0)
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
            if not with_rest:  # once more with a rest pose to leave untouched
                ctx.pose_parts([(0, 3, np.eye(3, 4))])  # (it tightens the loose boxes on its paths, which cull: the image to keep is the one from here on)
                img = render(ctx, cam, 2)
                s0 = ctx.scene_state()
                assert s0["rest"].shape == (tris.shape[0], 12)
        # the pose form's own refusals still come first
        with pytest.raises(native.NativeError, match="share triangle"):
            ctx.pose_parts([(0, 5, np.eye(3, 4)), (4, 2, np.eye(3, 4))], rebuild_above=gp.LIMIT)
        rep = ctx.pose_parts(moves, rebuild_above=math.inf)
        posed = scene.pose_parts(stored, moves)
        refit = scene.refit_bvh(scene.refit_bvh(loose, stored, touched=np.arange(3)), posed, touched=gp.listed_of(moves))  # (the identity pose above tightened its own paths)
        assert refit.tobytes() != scene.refit_bvh(loose, posed).tobytes()  # some box off the listed paths is still loose
        assert not rep.rebuilt and close(rep.cost, scene.tree_cost(refit)) and close(rep.base_cost, scene.tree_cost(loose))
        s1 = ctx.scene_state(["nodes", "tris"])
        assert ds.same_nodes(s1["nodes"], ds.device_layout(refit)[0]) and ds.same_bytes(s1["tris"], posed)
    finally:
        ctx.close()


# ---- brute force, frames in flight ---------------------------------------------------------------------------------------------------------------------------------

def test_brute_force_contexts_take_the_plain_pose(native):
    from rvpt_amd import scene
    tris, mats, cam = scene_of("default")
    moves = scene.part_moves([gp.turned(tris, 0, 63, 25.0)])
    a, b = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE), native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
    try:
        a.upload_scene(None, tris, mats)
        b.upload_scene(None, tris, mats)
        still = render(a, cam, 2)
        rc, msg = raw_pose(native, a, moves, native.nodes_update_pose_guarded(1100))
        assert rc == 0 and msg == ""
        assert a.pose_parts(moves, rebuild_above=gp.LIMIT) is None
        b.pose_parts(moves)
        got = render(a, cam, 2)
        assert np.array_equal(bits(got), bits(render(b, cam, 2))) and not np.array_equal(bits(got), bits(still))
    finally:
        a.close()
        b.close()


def test_frames_queued_before_the_call_finish_on_the_old_geometry(native, oracle):
    from rvpt_amd import RenderSettings
    name, method = "terrain16", "sah"
    tris, mats, cam = scene_of(name)
    st = built_of(name, method)
    first, count = gp.part_of(tris.shape[0])
    moves = [gp.carried(tris, first, count)]
    r = gp.step(st, moves, gp.LIMIT, method)
    assert r.rebuilt
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        for f in range(4):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        rep = ctx.pose_parts(moves, rebuild_above=gp.LIMIT)  # with four frames queued: posed, costed and rebuilt
        assert rep.rebuilt and ctx.query() is False
        img_old = ctx.read()
        img_new = render(ctx, cam, 2)
    finally:
        ctx.close()
    ref_old, _ = oracle_frames(oracle, (tris[st.perm], mats, st.nodes), cam, W, H, "bvh", [0, 1, 2, 3])
    ref_new, _ = oracle_frames(oracle, (r.state.current[r.state.perm], mats, r.state.nodes), cam, W, H, "bvh", [0, 1])
    assert np.array_equal(bits(img_old), bits(ref_old[3])) and np.array_equal(bits(img_new), bits(ref_new[1]))


# ---- mirrors ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_renderer_keyword_restates_its_host_tree_after_a_rebuild(native):
    from rvpt_amd import RVPT, scene
    tris, mats, _ = scene_of("terrain16")
    n = tris.shape[0]
    first, count = gp.part_of(n)
    r = RVPT(W, H, device=0, traversal="bvh", build="device-sah")
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        built = scene.build_sah(tris)
        turned = [gp.turned(tris, first, count, 2.0)]
        assert r.pose_parts(turned) is None
        rep = r.pose_parts(turned, rebuild_above=gp.LIMIT)
        assert not rep.rebuilt and rep.tree is None
        once = scene.pose_parts(tris, turned)
        assert np.array_equal(r.primitive_indices, built[1]) and np.array_equal(r.bvh_nodes, scene.refit_bvh(built[0], once[built[1]]))
        rep = r.pose_parts([gp.carried(tris, first, count)], rebuild_above=gp.LIMIT)
        assert rep.rebuilt and rep.tree == "sah"
        far = scene.pose_parts(tris, [gp.carried(tris, first, count)])
        nodes, perm = scene.build_sah(far)[:2]
        assert np.array_equal(r.bvh_nodes, nodes) and np.array_equal(r.primitive_indices, perm) and np.array_equal(r.sorted_triangles, far[perm])
        assert np.array_equal(np.concatenate(r.triangles), far)
        # its own rest copy, in added order, stays: the next pose starts from the triangles as they were added
        assert r.pose_parts(turned) is None
        assert np.array_equal(np.concatenate(r.triangles), once) and np.array_equal(r.sorted_triangles, once[perm])
        assert np.array_equal(r.bvh_nodes, scene.refit_bvh(nodes, once[perm]))
    finally:
        r.shutdown()


def test_a_ploc_rebuild_that_falls_back_reports_lbvh(native):
    """tests/test_ploc_host.py's nested triangles: PLOC's tree of them is too high, before the pose and after it"""
    from rvpt_amd import scene
    from test_ploc_host import nested_triangles
    tris = np.ascontiguousarray(nested_triangles())
    mats = scene.default_materials()
    info = {}
    nodes, perm = scene.build_ploc(tris, info=info)[:2]
    assert info["tree"] == "lbvh"
    st = gp.State(nodes, np.asarray(perm, dtype=np.int64), scene.tree_cost(nodes), tris, tris)
    moves = [(0, 1, np.diag([5e7, 5e7, 5e7]) @ np.eye(3, 4))]  # the innermost triangle blown up to the size of the outermost: the ratio is 1.577
    r = gp.step(st, moves, gp.LIMIT, "ploc")
    scene.build_ploc(r.state.current, info=info)
    assert r.rebuilt and info["tree"] == "lbvh" and r.cost / st.base > 1.5
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        assert ctx.build_scene(tris, mats, method="ploc") == "lbvh"
        rep = ctx.pose_parts(moves, rebuild_above=gp.LIMIT)
        assert rep.rebuilt and rep.tree == "lbvh" and close(rep.cost, r.cost) and close(rep.base_cost, st.base)
        assert " permille: rebuilt (lbvh), new base cost " in said(ctx)
        s = ctx.scene_state()
        assert s["built_by"] == "ploc"  # (rebuilt as PLOC, by the same rule, the next time too)
        assert ds.same_nodes(s["nodes"], ds.shifted_layout(r.state.nodes)) and ds.same_bytes(s["rest"], tris[r.state.perm][:, :12])
    finally:
        ctx.close()
