"""The guarded skin update on the GPU: rvpt_hip_upload_scene's RVPT_HIP_NODES_UPDATE_SKIN_GUARDED form (Context.skin(rebuild_above=)) skins every vertex from the
rest pose, refits every box, costs the stored tree and, past a limit, rebuilds it by the builder that made it — and the rest pose follows the triangles through
the rebuild while the binding stays where it is.  The reported numbers against the numpy statement of one step (tests/_guarded_skin.py) at 1e-9 relative;
everything else bit for bit: images, segment counts and launches against fresh contexts and the CPU oracle, and in the laboratory build the triangles, the
nodes, the wide form, the permutation, the rest pose, the binding and the matrices against the statement after every step."""
import ctypes
import math

import numpy as np
import pytest

import _device_state as ds
import _guarded_pose as gp
import _guarded_skin as gs
import _skin
from test_device_build import camera_for, native  # noqa: F401  (native: the module's fixture)
from test_device_state import same_state
from test_gpu_parity import oracle_frames
from test_refit import bits, flags_of, render, scene_and_camera

pytestmark = pytest.mark.gpu

W, H = 64, 48
REL = 1e-9  # double summation over n <= 2^21 terms in any order errs by at most n * 2^-53 = 2.3e-10 relative: the tolerance of the guarded pose update's test
NOT_THE_BUILDS = ("rest", "skin", "bones")  # what a context that skinned holds and a fresh build of the same triangles does not
_SCENES, _BUILT = {}, {}


def scene_of(name):
    """(tris in the generator's order, mats, camera) — made once, shared and left unchanged"""
    if name not in _SCENES:
        tris, mats = gs.tris_of(name)
        tris, mats = np.ascontiguousarray(tris), np.ascontiguousarray(mats)
        tris.setflags(write=False)
        _SCENES[name] = (tris, mats, camera_for({"cornell2": "cornell"}.get(name, name), W, H))
    return _SCENES[name]


def built_of(name, method, k=gs.N_BONES):
    if (name, method, k) not in _BUILT:
        tris = scene_of(name)[0]
        _BUILT[name, method, k] = gs.built(tris, method, gs.weights(tris, k))
    return _BUILT[name, method, k]


def close(a, b):
    return abs(a - b) <= REL * abs(b)


def said(ctx):
    return (ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode()


def raw(native, ctx, count, lst, n, tris=None, mats=None, offset=0):
    """the C call itself: (return code, message); lst: a numpy array, a device pointer (int) or None; count: the n_nodes argument; n: the n_tris argument"""
    keep = np.ascontiguousarray(lst) if isinstance(lst, np.ndarray) else None
    ptr = None if lst is None else ctypes.c_void_p((keep.ctypes.data if keep is not None else int(lst)) + offset)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=np.float32)
    mm = None if mats is None else np.ascontiguousarray(mats, dtype=np.float32)
    rc = ctx._L.rvpt_hip_upload_scene(ctx._h, ptr, count, None if t is None else t.ctypes.data_as(ctypes.c_void_p), n, None if mm is None else mm.ctypes.data_as(ctypes.c_void_p),
                                      0 if mm is None else mm.shape[0])
    return rc, said(ctx)


def usable(ratio, limit):
    """the device adds in another order than numpy: a case decides alike where its ratio is a thousandth or more away from the limit (tests/test_guarded_skin_host.py
    asserts it of every case here without a GPU)"""
    if abs(ratio / limit - 1.0) < 1e-3:
        pytest.fail(f"misconfigured case: the ratio {ratio:.6f} lies within a thousandth of the limit {limit}")


def check_against_statement(native, state, before, st, r, bones, what):
    """the laboratory read-back `state` after a step against the statement: r = gs.step(st, bones, ...); before: the read-back in front of the step"""
    from rvpt_amd import scene
    new = r.state
    dev = ds.shifted_layout(new.nodes)
    assert ds.same_nodes(state["nodes"], dev), (what, "d_nodes", ds.first_difference(state["nodes"], dev))
    assert ds.same_bytes(state["perm"], new.perm.astype(np.uint32)), (what, "d_perm")
    assert ds.same_bytes(state["tris"], new.current[new.perm]), (what, "d_tris", ds.first_difference(state["tris"], new.current[new.perm]))
    assert ds.same_bytes(state["rest"], new.rest[new.perm][:, :12]), (what, "REST is the old rest pose in the new stored order", ds.first_difference(state["rest"], new.rest[new.perm][:, :12]))
    assert state["skin"].dtype == native.VERTEX_SKIN_DTYPE and state["skin"].tobytes() == new.skin.tobytes(), (what, "SKIN is the binding, unchanged, in the caller's order")
    assert state["bones"].tobytes() == scene.bone_matrices(bones).tobytes(), (what, "BONES are the call's matrices")
    assert state["have_cost"] and state["have_perm"], what
    if r.rebuilt:
        assert close(state["base_cost"], new.base), (what, state["base_cost"], new.base)
    else:
        assert state["base_cost"] == before["base_cost"] and close(state["base_cost"], st.base), what
        want_wide = ds.regathered(before["wide"], before["wide_map"], dev)
        assert ds.same_bytes(state["wide"], want_wide), (what, "d_wide", ds.first_difference(state["wide"], want_wide))
        assert ds.same_bytes(state["wide_map"], before["wide_map"]) and ds.same_bytes(state["refit_levels"], before["refit_levels"]), what
    ds.check_wide_map(state, what)


def guarded_step(native, ctx, st, bones, limit, method, what, before=None, send=None):
    """one call and its statement: the report against the statement's numbers and decision, and the read-back where the context is a laboratory one.
    send: what goes to Context.skin in place of `bones` (the same matrices in another container)"""
    r = gs.step(st, bones, limit, method)
    if gs.permille_of(limit):
        usable(r.cost / st.base, gs.permille_of(limit) / 1000.0)
    if before is None and ctx.lab:
        before = ctx.scene_state()
    rep = ctx.skin(bones if send is None else send, rebuild_above=limit)
    print(f"{what}: device {said(ctx)}; numpy cost {r.cost!r}, base {st.base!r}, ratio {r.cost / st.base:.6f}, rebuilt {r.rebuilt}")
    assert close(rep.cost, r.cost), (what, rep.cost, r.cost)
    assert close(rep.base_cost, st.base), (what, rep.base_cost, st.base)
    assert rep.rebuilt == r.rebuilt and rep.tree == (method if r.rebuilt else None), (what, rep)
    if r.rebuilt:
        new_base = float(said(ctx).rsplit("new base cost ", 1)[1])
        assert close(new_base, r.state.base), (what, new_base, r.state.base)
    state = None
    if ctx.lab:
        state = ctx.scene_state()
        check_against_statement(native, state, before, st, r, bones, what)
    return r, rep, state


def bound(native, name, method, fl=None, lab=True, k=gs.N_BONES):
    """a context holding build_scene(name, method) and the binding of built_of(name, method, k)"""
    tris, mats, _ = scene_of(name)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH if fl is None else fl, lab=lab)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        ctx.bind_skin(built_of(name, method, k).skin)
    except BaseException:
        ctx.close()
        raise
    return ctx


# ---- the count is a form ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_count_is_a_form_of_the_call(native, method):
    """until this form existed the count fell through to the other forms, which refused it"""
    from rvpt_amd import scene
    tris = scene_of("cornell2")[0]
    ctx = bound(native, "cornell2", method, lab=False)
    try:
        rc, msg = raw(native, ctx, native.nodes_update_skin_guarded(0), scene.bone_matrices(gs.gentle(tris)), gs.N_BONES)
        assert rc == 0, msg
        assert msg.startswith("guarded skin update: cost ") and msg.endswith(", limit 0 permille: refitted")
        rep = native.parse_update_report(msg)
        assert rep.cost > 1.0 and rep.base_cost > 1.0 and not rep.rebuilt
    finally:
        ctx.close()


# ---- numbers --------------------------------------------------------------------------------------------------------------------------------------------------

NUMBER_CASES = [(n, m) for n in ("terrain16", "cornell2") for m in gs.METHODS]


@pytest.mark.parametrize("name,method", NUMBER_CASES, ids=[f"{n}-{m}" for n, m in NUMBER_CASES])
def test_the_reported_numbers_are_the_statements(native, name, method):
    """cost and base cost of a report, and after a rebuild the new base cost, at 1e-9 relative; %.17g brings the doubles back as they were"""
    tris = scene_of(name)[0]
    st = built_of(name, method)
    ctx = bound(native, name, method, lab=False)
    try:
        r, rep, _ = guarded_step(native, ctx, st, gs.gentle(tris), math.inf, method, f"{name} {method} gentle")
        first_said = said(ctx)
        assert rep.ratio == rep.cost / rep.base_cost
        assert first_said == f"guarded skin update: cost {rep.cost:.17g}, base cost {rep.base_cost:.17g}, limit 0 permille: refitted"
        ctx.skin(gs.gentle(tris), rebuild_above=math.inf)
        assert said(ctx) == first_said, "the same tree must give the same 64 bits on every run"
        r2, rep2, _ = guarded_step(native, ctx, r.state, gs.carrying(tris), gs.LIMIT, method, f"{name} {method} carrying")
        assert r2.rebuilt and f", limit 1100 permille: rebuilt ({method}), new base cost " in said(ctx)
        r3, rep3, _ = guarded_step(native, ctx, r2.state, gs.gentle(tris, phase=2.0), math.inf, method, f"{name} {method} gentle on the new tree")
        assert close(rep3.base_cost, r2.state.base) and not rep3.rebuilt
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
    ctx = bound(native, name, method, fl=fl)
    decisions = []
    try:
        before = ctx.scene_state()
        assert before["skin"].tobytes() == st.skin.tobytes() and before["rest"].size == 0
        still = render(ctx, cam, 2, batch=batch)
        seen, info = ctx.stats(), ctx.launch_info()[:3]
        if path is not None:
            assert info[2] == path
        for j, bones in enumerate(gs.sequence(tris)):
            what = f"{name} {method} {traversal} step {j + 1}"
            r, rep, state = guarded_step(native, ctx, st, bones, gs.LIMIT, method, what, before=before)
            decisions.append(r.rebuilt)
            got = render(ctx, cam, 2, batch=batch)
            now = ctx.stats()
            new = r.state
            stored = new.current[new.perm]
            if r.rebuilt:  # the context holds what a fresh build of the skinned triangles holds, the rest pose, the binding and the matrices apart
                want, want_stats, want_info, want_state = fresh_of(native, fl, lambda c: c.build_scene(new.current, mats, method=method), cam, batch)
                same_state(state, want_state, but=NOT_THE_BUILDS)
                assert ctx.launch_info()[:3] == want_info, (what, ctx.launch_info()[:3], want_info)
            else:  # ... or what an upload of the statement's refit holds
                want, want_stats, want_info, _ = fresh_of(native, fl, lambda c: c.upload_scene(new.nodes, stored, mats), cam, batch)
                # the kernel path is the fresh upload's; the LDS bytes follow the grouping of the wide form, which a refit keeps from the build and a fresh upload of
                # the moved tree may make anew (include/rvpt_hip.h: SKIN UPDATE), so they stay the context's own
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
@pytest.mark.parametrize("name", ["terrain16", "cornell2"])
def test_the_sequence(native, oracle, name, method, traversal):
    """refit, rebuild, refit, rebuild — steps three and four skin from the rest pose through the permutation step two made (512 and 2300 triangles)"""
    assert run_sequence(native, oracle, name, method, traversal, False) == [False, True, False, True]


def test_the_sequence_on_the_hbm_resident_wide_walk(native, oracle, monkeypatch):
    monkeypatch.setenv("RVPT_HIP_BVH_NO_RESIDENT", "1")
    assert run_sequence(native, oracle, "terrain16", "sah", "bvh", False, path=10) == [False, True, False, True]


@pytest.mark.parametrize("name,method", [("terrain16", "ploc"), ("cornell2", "sah")])
def test_the_sequence_in_batched_launches(native, oracle, name, method):
    assert run_sequence(native, oracle, name, method, "bvh", True) == [False, True, False, True]


# ---- afterwards -------------------------------------------------------------------------------------------------------------------------------------------------

def test_after_a_rebuild_every_form_answers_by_the_statement(native):
    from rvpt_amd import scene
    name, method = "terrain16", "sah"
    tris, mats, cam = scene_of(name)
    n = tris.shape[0]
    st = built_of(name, method)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a = bound(native, name, method, fl=fl)
    b = native.Context(W, H, 0, 0, 1, fl, lab=True)

    def alike(what, but=NOT_THE_BUILDS):
        sa, sb = a.scene_state(), b.scene_state()
        same_state(sa, sb, but=but)
        assert np.array_equal(bits(render(a, cam, 2)), bits(render(b, cam, 2))), what
        return sa, sb

    try:
        r, _, _ = guarded_step(native, a, st, gs.carrying(tris), gs.LIMIT, method, "carrying")
        assert r.rebuilt
        at_rebuild, perm = r.state.current, r.state.perm
        assert b.build_scene(at_rebuild, mats, method=method) == method
        alike("rebuilt")
        # read_triangles: the skinned rows in the caller's order; closest_points: prim numbers the caller's order on both
        assert ds.same_bytes(a.read_triangles(), at_rebuild)
        rng = np.random.RandomState(5)
        points = (rng.uniform(-4.0, 4.0, size=(200, 3)) * np.array([1.0, 0.3, 1.0])).astype(np.float32)
        ca, cb = a.closest_points(points), b.closest_points(points)
        assert ca.tobytes() == cb.tobytes() and int(ca["prim"].max()) < n
        # a plain skin with other bones: from the rest pose of before the rebuild, through the same weights; on the fresh build the same vertices by a plain update
        other = _skin.bones(tris, gs.N_BONES, 0.7)
        skinned = scene.skin_triangles(tris, st.skin, other)
        assert a.skin(other) is None and said(a) == ""
        b.update_triangles(skinned)
        sa, _ = alike("a plain skin after the rebuild")
        assert ds.same_bytes(sa["tris"], skinned[perm]) and ds.same_bytes(sa["rest"], tris[perm][:, :12]) and sa["skin"].tobytes() == st.skin.tobytes()
        assert sa["bones"].tobytes() == scene.bone_matrices(other).tobytes()
        # a pose of one part: from the same rest pose, the other rows as the skin left them
        first, count = gp.part_of(n)
        moves = [gp.turned(tris, first, count, 3.0)]
        posed = scene.pose_parts(tris, moves, current=skinned)
        assert a.pose_parts(moves) is None
        idx = gp.listed_of(moves)
        b.update_triangles(posed[idx], indices=idx)
        sa, _ = alike("a pose after the rebuild")
        assert ds.same_bytes(sa["tris"], posed[perm]) and ds.same_bytes(sa["rest"], tris[perm][:, :12]) and sa["skin"].tobytes() == st.skin.tobytes()
        # a guarded pose: the statement of the guarded pose update on the tree as it stands — every box tight, so its refit of the listed paths is the full one
        pst = gp.State(scene.refit_bvh(r.state.nodes, posed[perm]), perm, r.state.base, tris, posed)
        carried = [gp.carried(tris, first, count)]
        pr = gp.step(pst, carried, None, method)  # (report only, as every call below: no decision of this test but the first is taken near a limit)
        rep = a.pose_parts(carried, rebuild_above=math.inf)
        assert close(rep.cost, pr.cost) and close(rep.base_cost, pst.base) and not rep.rebuilt
        sa = a.scene_state()
        new = pr.state
        assert ds.same_nodes(sa["nodes"], ds.shifted_layout(new.nodes)) and ds.same_bytes(sa["perm"], new.perm.astype(np.uint32))
        assert ds.same_bytes(sa["tris"], new.current[new.perm]) and ds.same_bytes(sa["rest"], tris[new.perm][:, :12]) and sa["skin"].tobytes() == st.skin.tobytes()
        # ... and the skin after it poses from the rest pose through the permutation as it now stands
        gst = gs.State(new.nodes, new.perm, new.base, tris, new.current, st.skin)
        r2, _, _ = guarded_step(native, a, gst, gs.gentle(tris, phase=1.3), math.inf, method, "gentle after a guarded pose")
        # a sparse update, numbered in the caller's order: the rest pose goes, as after every other form, and the next skin snapshots afresh
        rows = scene.wobble(r2.state.current, 0.7, 0.05)[10:40]
        a.update_triangles(rows, indices=np.arange(10, 40))
        assert a.scene_state(["rest"])["rest"].size == 0 and a.scene_state(["skin"])["skin"].tobytes() == st.skin.tobytes()
        moved = r2.state.current.copy()
        moved[10:40, :12] = rows[:, :12]
        held = scene.refit_bvh(r2.state.nodes, moved[r2.state.perm])
        r3, _, _ = guarded_step(native, a, gs.State(held, r2.state.perm, r2.state.base, moved, moved, st.skin), gs.gentle(tris, phase=0.2), math.inf, method, "gentle after a sparse update")
        # a plain update in the caller's order: the same
        moved = scene.wobble(tris, 1.9, 0.05)
        a.update_triangles(moved)
        assert a.scene_state(["rest"])["rest"].size == 0
        held = scene.refit_bvh(r3.state.nodes, moved[r3.state.perm])
        r4, _, _ = guarded_step(native, a, gs.State(held, r3.state.perm, r3.state.base, moved, moved, st.skin), gs.carrying(tris), math.inf, method, "carrying after a plain update")
        # a second bind replaces the first and keeps the rest pose
        rec2 = gs.weights(tris, 5)
        a.bind_skin(rec2)
        r5, _, _ = guarded_step(native, a, r4.state._replace(skin=rec2), _skin.bones(tris, 5), math.inf, method, "after a second bind")
        # a full upload drops the binding: the guarded count then says what the plain one says
        a.build_scene(tris, mats, method=method)
        rc, msg = raw(native, a, native.nodes_update_skin_guarded(1100), scene.bone_matrices(_skin.bones(tris, 5)), 5)
        assert rc == native.ERR_INVALID and "skin update before a bind" in msg
        # ... and so does an ordinary upload of nodes and triangles, after a bind that the build form's scene took
        a.bind_skin(rec2)
        assert a.scene_state(["skin"])["skin"].tobytes() == rec2.tobytes()
        a.upload_scene(st.nodes, tris[st.perm], mats)
        assert a.scene_state(["skin"])["skin"].size == 0
        for permille in (0, 1100):
            rc, msg = raw(native, a, native.nodes_update_skin_guarded(permille), scene.bone_matrices(_skin.bones(tris, 5)), 5)
            assert rc == native.ERR_INVALID and "skin update before a bind" in msg
    finally:
        a.close()
        b.close()


# ---- shapes -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
@pytest.mark.parametrize("k", gs.SHAPE_BONES)  # 1024: the full 48 KiB of LDS
def test_bone_counts_on_the_default_scene(native, k, method):
    """143 triangles: 429 vertices, the last wave partial.  With one bone the mesh moves as one, with three it bends as a whole (two refits); 1024 bones rebuild"""
    name = "default"
    tris, mats, cam = scene_of(name)
    st = built_of(name, method, k)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = bound(native, name, method, fl=fl, k=k)
    try:
        decisions = []
        for j, bones in enumerate(gs.shape_steps(tris, k)):
            r, _, state = guarded_step(native, ctx, st, bones, gs.LIMIT, method, f"default {k} bones {method} call {j + 1}")
            assert state["bones"].shape == (k, 12)
            decisions.append(r.rebuilt)
            new = r.state
            got = render(ctx, cam, 2)
            if r.rebuilt:
                want, _, want_info, want_state = fresh_of(native, fl, lambda c: c.build_scene(new.current, mats, method=method), cam, False)
                same_state(state, want_state, but=NOT_THE_BUILDS)
                assert ctx.launch_info()[:3] == want_info
            else:
                want, _, _, _ = fresh_of(native, fl, lambda c: c.upload_scene(new.nodes, new.current[new.perm], mats), cam, False)
            assert np.array_equal(bits(got), bits(want))
            st = new
        assert decisions == [False, k == 1024]
    finally:
        ctx.close()


def test_the_sequence_on_the_default_scene(native):
    """the decisions are the statement's (refit, rebuild, refit, rebuild in numpy: tests/_guarded_skin.py: gpu_ratios)"""
    name, method = "default", "ploc"
    tris = scene_of(name)[0]
    st = built_of(name, method)
    ctx = bound(native, name, method)
    try:
        for j, bones in enumerate(gs.sequence(tris)):
            r, _, _ = guarded_step(native, ctx, st, bones, gs.LIMIT, method, f"default {method} step {j + 1}")
            st = r.state
    finally:
        ctx.close()


def test_bones_from_a_device_tensor_give_the_host_arrays_bytes(native):
    import torch
    from rvpt_amd import scene
    name, method = "cornell2", "lbvh"
    tris = scene_of(name)[0]
    st = built_of(name, method)
    a, b = bound(native, name, method), bound(native, name, method)
    try:
        for bones, limit in ((gs.gentle(tris), math.inf), (gs.carrying(tris), gs.LIMIT)):
            dev = torch.from_numpy(scene.bone_matrices(bones).copy()).to("cuda:0")
            r, rep_a, sa = guarded_step(native, a, st, bones, limit, method, "host bones")
            _, rep_b, sb = guarded_step(native, b, st, bones, limit, method, "device bones", send=dev)
            assert rep_a == rep_b
            same_state(sa, sb)
            st = r.state
        assert r.rebuilt
    finally:
        a.close()
        b.close()


def test_67712_triangles_and_1024_bones_rebuilt_once(native):
    """tests/test_skin_update.py's mesh larger than one grid of skin work-groups, its random influences, and a rebuild behind it"""
    tris, mats, rec, bones = gs.big_case()
    n = tris.shape[0]
    assert n == 67712
    st = gs.built(tris, "lbvh", rec)
    a, b = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True), native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        a.build_scene(tris, mats, method="lbvh")
        a.bind_skin(rec)
        r = gs.step(st, bones, gs.LIMIT, "lbvh")
        usable(r.cost / st.base, gs.LIMIT)
        rep = a.skin(bones, rebuild_above=gs.LIMIT)
        assert r.rebuilt and rep.rebuilt and rep.tree == "lbvh" and close(rep.cost, r.cost) and close(rep.base_cost, st.base)
        b.build_scene(r.state.current, mats, method="lbvh")
        pieces = ["tris", "nodes", "wide", "perm"]
        sa, sb = a.scene_state(pieces + ["rest", "skin"]), b.scene_state(pieces)
        for k in pieces:
            assert ds.same_bytes(sa[k], sb[k]), k
        assert close(sa["base_cost"], r.state.base) and sa["base_cost"] == sb["base_cost"]
        perm = sa["perm"].astype(np.int64)
        assert ds.same_bytes(sa["tris"], r.state.current[perm]) and ds.same_bytes(sa["rest"], tris[perm][:, :12]) and sa["skin"].tobytes() == rec.tobytes()
    finally:
        a.close()
        b.close()


def test_frames_queued_before_the_call_finish_on_the_old_geometry(native, oracle):
    from rvpt_amd import RenderSettings
    name, method = "terrain16", "sah"
    tris, mats, cam = scene_of(name)
    st = built_of(name, method)
    bones = gs.carrying(tris)
    r = gs.step(st, bones, gs.LIMIT, method)
    assert r.rebuilt
    ctx = bound(native, name, method, lab=False)
    try:
        for f in range(4):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        rep = ctx.skin(bones, rebuild_above=gs.LIMIT)  # with four frames queued: skinned, costed and rebuilt
        assert rep.rebuilt and ctx.query() is False
        img_old = ctx.read()
        img_new = render(ctx, cam, 2)
    finally:
        ctx.close()
    ref_old, _ = oracle_frames(oracle, (tris[st.perm], mats, st.nodes), cam, W, H, "bvh", [0, 1, 2, 3])
    ref_new, _ = oracle_frames(oracle, (r.state.current[r.state.perm], mats, r.state.nodes), cam, W, H, "bvh", [0, 1])
    assert np.array_equal(bits(img_old), bits(ref_old[3])) and np.array_equal(bits(img_new), bits(ref_new[1]))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

PIECES = ["tris", "nodes", "rest", "wide", "skin", "bones"]


def test_refusals_leave_the_scene_the_rest_pose_and_the_binding_untouched(native):
    """every refusal of the plain skin form, in its order and its words, reached through the guarded count; then the band's own"""
    import torch
    name, method = "default", "sah"
    tris, mats, cam = scene_of(name)
    n = tris.shape[0]
    rec = gs.weights(tris, 7)
    m = _skin.bones(tris, 7).reshape(7, 12)
    top = int(rec["bone"].max())
    top_pos = int(np.argwhere(rec["bone"] == top)[0][0])
    assert top == 6
    count = native.nodes_update_skin_guarded(1100)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        rc, msg = raw(native, ctx, count, None, 0)
        assert rc == native.ERR_INVALID and "skin update before any full upload_scene" in msg
        assert ctx.build_scene(tris, mats, method=method) == method
        rc, msg = raw(native, ctx, count, m, 7)
        assert rc == native.ERR_INVALID and "skin update before a bind" in msg
        ctx.bind_skin(rec)
        ctx.skin(m, rebuild_above=math.inf)  # so that there is a rest pose to leave untouched
        img = render(ctx, cam, 2)
        s0 = ctx.scene_state()
        assert s0["rest"].shape == (n, 12) and s0["skin"].tobytes() == rec.tobytes() and s0["bones"].shape == (7, 12)

        def untouched(what):
            same_state(ctx.scene_state(), s0)
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img)), what

        d_m = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), m.reshape(-1)])).to("cuda:0")
        assert d_m.data_ptr() % 16 == 0
        big = np.zeros((1025, 12), dtype=np.float32)
        cases = [((None, 0, tris[:1]), "skin update without bones"),  # each offends at its own place and at later ones: the message is the earlier one's
                 ((None, 1025, tris[:1]), "skin update with 1025 bones: at most 1024"),
                 ((None, 6, tris[:1]), "skin update without a list"),
                 ((big, 6, tris[:1], None, 2), "is not 4-byte aligned"),
                 ((d_m.data_ptr() + 4, 6, tris[:1]), "is not 16-byte aligned"),
                 ((m, 6, tris[:1], mats), "skin update takes no triangles"),
                 ((m, 6, None, mats), "skin update takes no materials"),
                 ((m, 6), f"skin update with 6 bones: the binding names bone 6 (skin[{top_pos}]), which needs 7"),
                 ((d_m.data_ptr() + 16, 6), f"skin update with 6 bones: the binding names bone 6 (skin[{top_pos}]), which needs 7")]
        for args, what in cases:
            rc, msg = raw(native, ctx, count, *args)
            assert rc == native.ERR_INVALID and what in msg, (what, rc, msg)
            untouched(what)
        if torch.cuda.device_count() > 1:  # another GPU's memory is refused, naming both devices; it comes behind the count of bones
            other = torch.from_numpy(m.copy()).to("cuda:1")
            rc, msg = raw(native, ctx, count, other.data_ptr(), 7)
            assert rc == native.ERR_INVALID and "device memory of GPU 1, the context lives on GPU 0" in msg
            untouched("another GPU's memory")
            rc, msg = raw(native, ctx, count, other.data_ptr(), 6)
            assert rc == native.ERR_INVALID and "the binding names bone 6" in msg
            untouched("another GPU's memory, too few bones")
        for permille in (1, 999, 65536, 0xFFFFF):  # ... and the one of the band, which comes before them all
            rc, msg = raw(native, ctx, native.nodes_update_skin_guarded(permille), None, 0, tris[:1])
            assert rc == native.ERR_INVALID and msg == f"guarded skin update: the limit is 0 (report only) or 1000 .. 65535 permille, got {permille}", msg
            untouched(msg)
        for bad in (0.5, float("nan"), 70, -1):
            with pytest.raises(native.NativeError, match="rebuild_above"):
                ctx.skin(m, rebuild_above=bad)
        with pytest.raises(native.NativeError, match="the binding names bone 6"):
            ctx.skin(m[:6], rebuild_above=gs.LIMIT)
        untouched("the wrapper's refusals")
        for permille in (1000, 65535):  # the band's ends are forms of the call
            rc, msg = raw(native, ctx, native.nodes_update_skin_guarded(permille), m, 7)
            assert rc == 0 and f"limit {permille} permille: " in msg, msg
    finally:
        ctx.close()


def test_after_an_ordinary_upload_a_limit_is_refused_and_a_report_is_legal(native):
    """the tree is the caller's: a limit has no builder to name; report only skins, refits every box, reports and never rebuilds"""
    from rvpt_amd import scene
    tris, mats, cam = scene_of("default")
    built = gs.built(tris, "sah", gs.weights(tris))
    stored = tris[built.perm]
    rec = gs.weights(stored)  # (after an ordinary upload the records are in the leaf order of that upload)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(built.nodes, stored, mats)
        ctx.bind_skin(rec)
        img = render(ctx, cam, 2)
        s0 = ctx.scene_state()
        bones = gs.carrying(tris)
        for with_rest in (False, True):
            with pytest.raises(native.NativeError, match="guarded skin update with a limit after an ordinary upload_scene.*no builder") as e:
                ctx.skin(bones, rebuild_above=gs.LIMIT)
            assert e.value.code == native.ERR_INVALID
            same_state(ctx.scene_state(), s0)
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
            if not with_rest:  # once more with a rest pose and matrices to leave untouched
                ctx.skin(gs.gentle(tris))
                img = render(ctx, cam, 2)
                s0 = ctx.scene_state()
                assert s0["rest"].shape == (tris.shape[0], 12)
        # the skin form's own refusals still come first
        with pytest.raises(native.NativeError, match="skin update with 3 bones: the binding names bone"):
            ctx.skin(bones[:3], rebuild_above=gs.LIMIT)
        # report only: the carrying set, 1.2 times the base in numpy, is reported and refitted
        rep = ctx.skin(bones, rebuild_above=math.inf)
        skinned = scene.skin_triangles(stored, rec, bones)
        refit = scene.refit_bvh(built.nodes, skinned)
        assert not rep.rebuilt and rep.tree is None and close(rep.cost, scene.tree_cost(refit)) and close(rep.base_cost, built.base) and rep.ratio > gs.LIMIT
        s1 = ctx.scene_state(["nodes", "tris", "rest", "skin"])
        assert ds.same_nodes(s1["nodes"], ds.device_layout(refit)[0]) and ds.same_bytes(s1["tris"], skinned)
        assert ds.same_bytes(s1["rest"], stored[:, :12]) and s1["skin"].tobytes() == rec.tobytes()
    finally:
        ctx.close()


def test_caller_layout_has_no_guarded_skin_form(native, monkeypatch):
    """the last refusal of the skin form, the laboratory's caller-layout knob, under the guarded count: the plain form's answer, and nothing touched"""
    from rvpt_amd import scene
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    (stored, mats, nodes), cam = scene_and_camera("default", W, H)  # (rvpt_bvh_build's tree and its leaf order, as tests/test_skin_update.py uploads them)
    rec = gs.weights(stored, 3)
    m = scene.bone_matrices(_skin.bones(stored, 3))
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(nodes, stored, mats)
        for permille in (0, 1100):
            rc, msg = raw(native, ctx, native.nodes_update_skin_guarded(permille), m, 3)
            assert rc == native.ERR_INVALID and "skin update before a bind" in msg  # (the earlier refusal)
        ctx.bind_skin(rec)
        img = render(ctx, cam, 1)
        pieces = ["tris", "nodes", "rest", "skin", "bones"]
        s0 = ctx.scene_state(pieces)
        for permille in (0, 1100):  # (1100 on an ordinary upload: the form's own refusal would come behind this one)
            rc, msg = raw(native, ctx, native.nodes_update_skin_guarded(permille), m, 3)
            assert rc == native.ERR_UNSUPPORTED and "CALLER_LAYOUT" in msg, (rc, msg)
            with pytest.raises(native.NativeError, match="CALLER_LAYOUT") as e:
                ctx.skin(m, rebuild_above=math.inf if permille == 0 else gs.LIMIT)
            assert e.value.code == native.ERR_UNSUPPORTED
            s = ctx.scene_state(pieces)
            for k in pieces:
                assert ds.same_bytes(s[k], s0[k]), k
            assert s["rest"].size == 0 and s["skin"].tobytes() == rec.tobytes()
            assert np.array_equal(bits(render(ctx, cam, 1)), bits(img))
    finally:
        ctx.close()


# ---- brute force ------------------------------------------------------------------------------------------------------------------------------------------------

def test_brute_force_contexts_take_the_plain_skin(native):
    import torch
    from rvpt_amd import scene
    tris, mats, cam = scene_of("default")
    rec = gs.weights(tris, 7)
    m = scene.bone_matrices(_skin.bones(tris, 7))
    a, b = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE, lab=True), native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
    try:
        for ctx in (a, b):
            ctx.upload_scene(None, tris, mats)
            ctx.bind_skin(rec)
        still = render(a, cam, 2)
        rc, msg = raw(native, a, native.nodes_update_skin_guarded(1100), m, 7)
        assert rc == 0 and msg == ""
        assert a.skin(m, rebuild_above=gs.LIMIT) is None
        b.skin(m)
        got = render(a, cam, 2)
        assert np.array_equal(bits(got), bits(render(b, cam, 2))) and not np.array_equal(bits(got), bits(still))
        # the skin form's refusal of a device pointer there, under the guarded count: the triangles, the rest pose and the binding, all on the host, stay
        pieces = ["tris", "rest", "skin", "bones"]
        s0 = a.scene_state(pieces)
        assert s0["rest"].shape == (tris.shape[0], 12) and s0["skin"].tobytes() == rec.tobytes()
        d_m = torch.from_numpy(_skin.bones(tris, 7, 0.9).reshape(7, 12).copy()).to("cuda:0")
        for permille in (0, 1100):
            rc, msg = raw(native, a, native.nodes_update_skin_guarded(permille), d_m.data_ptr(), 7)
            assert rc == native.ERR_INVALID and "skin update of a brute-force context from a device pointer" in msg, (rc, msg)
            s = a.scene_state(pieces)
            for k in pieces:
                assert ds.same_bytes(s[k], s0[k]), k
            assert np.array_equal(bits(render(a, cam, 2)), bits(got))
    finally:
        a.close()
        b.close()


# ---- mirrors ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_renderer_keyword_restates_its_host_tree_after_a_rebuild(native):
    from rvpt_amd import RVPT, scene
    tris, mats, _ = scene_of("terrain16")
    rec = built_of("terrain16", "sah").skin
    pair = []
    for _ in range(2):
        r = RVPT(W, H, device=0, traversal="bvh", build="device-sah")
        pair.append(r)
    a, b = pair

    def frames():
        out = []
        for r in pair:
            r.update()
            r.draw()
            r.update()
            r.draw()
            out.append(r.read_frame())
        return out

    try:
        a.add_triangles(tris)
        for m in mats:
            a.add_material(m)
        a.initialize()
        a.bind_skin(rec)
        built = scene.build_sah(tris)
        gentle, carrying = gs.gentle(tris), gs.carrying(tris)
        assert a.skin(gentle) is None
        rep = a.skin(gentle, rebuild_above=gs.LIMIT)
        assert not rep.rebuilt and rep.tree is None
        once = scene.skin_triangles(tris, rec, gentle)
        assert np.array_equal(a.primitive_indices, built[1]) and np.array_equal(a.bvh_nodes, scene.refit_bvh(built[0], once[built[1]]))
        rep = a.skin(carrying, rebuild_above=gs.LIMIT)
        assert rep.rebuilt and rep.tree == "sah"
        far = scene.skin_triangles(tris, rec, carrying)
        nodes, perm = scene.build_sah(far)[:2]
        assert np.array_equal(a.bvh_nodes, nodes) and np.array_equal(a.primitive_indices, perm) and np.array_equal(a.sorted_triangles, far[perm])
        assert np.array_equal(np.concatenate(a.triangles), far)
        # a second object built from the skinned triangles holds the same tree: the frames agree, and after the next skin — from the triangles as they were ADDED,
        # through the binding as it was bound — they agree with its plain update
        b.add_triangles(far)
        for m in mats:
            b.add_material(m)
        b.initialize()
        got, want = frames()
        assert np.array_equal(bits(got), bits(want))
        st = gs.step(gs.State(nodes, np.asarray(perm, dtype=np.int64), scene.tree_cost(nodes), tris, far, rec), gentle, gs.LIMIT, "sah")
        usable(st.cost / scene.tree_cost(nodes), gs.LIMIT)  # (tests/_guarded_skin.py: gpu_ratios restates this call, as it does the two before it)
        rep = a.skin(gentle, rebuild_above=gs.LIMIT)
        assert not rep.rebuilt and not st.rebuilt and close(rep.cost, st.cost) and close(rep.base_cost, scene.tree_cost(nodes))
        b.update_triangles(once)
        got, want = frames()
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(np.concatenate(a.triangles), once) and np.array_equal(a.sorted_triangles, once[perm])
        assert np.array_equal(a.bvh_nodes, st.state.nodes) and np.array_equal(a.bvh_nodes, scene.refit_bvh(nodes, once[perm]))
    finally:
        a.shutdown()
        b.shutdown()
