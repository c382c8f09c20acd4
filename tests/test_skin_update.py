"""The bind and the skin update on the GPU: rvpt_hip_upload_scene's RVPT_HIP_NODES_BIND_SKIN form (Context.bind_skin) keeps four bone indices and four weights
per vertex on the device, its RVPT_HIP_NODES_UPDATE_SKIN form (Context.skin) poses every vertex from the rest pose by its weighted matrices and refits every box.
Everything here is bit-exact: after an update the context renders what a fresh context given upload_scene(refit_bvh(nodes, skinned), skinned, mats) renders and
what the CPU oracle renders on that tree, with skinned = scene.skin_triangles(...), and the laboratory build's read-back shows the bytes the numpy statements
give.  No tolerance anywhere.  All at 64 x 48, two frames."""
import ctypes

import numpy as np
import pytest

import _device_state as ds
import _ray_query as rq
import _skin
from test_gpu_parity import oracle_frames
from test_pose_host import about, rotation
from test_refit import bits, flags_of, render, scene_and_camera

pytestmark = pytest.mark.gpu

W, H = 64, 48


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


@pytest.fixture(scope="module")
def cornell2():
    """cornell_scene(2): 2300 triangles, 6900 vertex quads = 27 work-groups of skin_vertices, in an order that is no leaf order, with its camera"""
    from rvpt_amd import Camera, scene
    tris, mats = scene.cornell_scene(2)
    assert tris.shape[0] == 2300 and _skin.no_minus_zero(tris)
    tris = tris[np.random.RandomState(17).permutation(tris.shape[0])]  # the caller's order: any order
    c = Camera(W / H)
    c.translation = np.array([0.0, 2.0, -1.9])
    for a in (tris, mats):
        a.setflags(write=False)
    return tris, mats, c.get_data()


def statement(tris, k, phase=0.0):
    """(records, matrices, skinned) of the generator for k bones; the skinned vertices hold no -0, the condition under which byte equality of boxes is defined"""
    from rvpt_amd import scene
    rec, m = _skin.weights(tris, k), _skin.bones(tris, k, phase)
    skinned = scene.skin_triangles(tris, rec, m)
    assert _skin.no_minus_zero(skinned) and np.isfinite(skinned[:, :12]).all() and not np.array_equal(bits(skinned[:, :12]), bits(tris[:, :12]))
    return rec, m, skinned


def fresh(native, fl, nodes, tris, mats, cam, batch=False, lab=None):
    ctx = native.Context(W, H, 0, 0, 1, fl, lab=lab)
    try:
        ctx.upload_scene(nodes, tris, mats)
        return render(ctx, cam, 2, batch=batch), ctx.stats(), ctx.launch_info()
    finally:
        ctx.close()


def last_error(ctx):
    return (ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode()


# ---- the default scene: 143 triangles, 429 threads — a partial last wave, a triangle split across two work-groups ------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 1024])  # 1024: 12 288 words staged by 256 threads, the full 48 KiB of LDS
@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("traversal,knob", [("bvh", None), ("bvh_ordered", None), ("bvh", "RVPT_HIP_BVH_NO_RESIDENT")])
def test_bind_and_skin_render_as_a_fresh_upload_of_the_refit_tree(native, oracle, monkeypatch, traversal, knob, batch, k):
    from rvpt_amd import scene
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    assert tris.shape[0] == 143 and _skin.no_minus_zero(tris)
    rec, m, skinned = statement(tris, k)
    refit = scene.refit_bvh(nodes, skinned)
    lab = None
    if knob:  # the HBM-resident wide walk on a scene that would fit LDS
        monkeypatch.setenv(knob, "1")
        lab = True
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS)
    ctx = native.Context(W, H, 0, 0, 1, fl, lab=lab)
    try:
        ctx.upload_scene(nodes, tris, mats)
        before = render(ctx, cam, 2, batch=batch)
        info, seen = ctx.launch_info(), ctx.stats()
        assert ctx.bind_skin(rec) is None and last_error(ctx) == ""
        bound = render(ctx, cam, 2, batch=batch)  # a bind moves nothing: the frame without it, bit for bit
        now = ctx.stats()
        assert np.array_equal(bits(bound), bits(before)) and (now[0] - seen[0], now[1] - seen[1]) == seen and ctx.launch_info() == info
        seen = now
        assert ctx.skin(m) is None and last_error(ctx) == ""
        got = render(ctx, cam, 2, batch=batch)
        now = ctx.stats()
        launch = ctx.launch_info()
    finally:
        ctx.close()
    want, want_stats, want_info = fresh(native, fl, refit, skinned, mats, cam, batch=batch, lab=lab)
    ref, seg = oracle_frames(oracle, (skinned, mats, refit), cam, W, H, traversal, [0, 1])
    assert not np.array_equal(bits(got), bits(before)), "the geometry did not move"
    assert np.array_equal(bits(got), bits(want)), "skin update != fresh upload of the refit tree"
    assert np.array_equal(bits(got), bits(ref[1])), "skin update != oracle"
    assert (now[0] - seen[0], now[1] - seen[1]) == want_stats and want_stats[0] == seg
    # the kernel path is the fresh upload's; the LDS bytes stay the context's own: they follow the wide form's grouping, which every update form keeps
    assert launch[2] == info[2] == want_info[2] and launch[1] == info[1]


# ---- cornell_scene(2) after each build form: a permutation in the way ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_after_build_scene_the_records_are_in_the_callers_order(native, cornell2, method):
    """Bound in the caller's order and skinned twice with different bones: equal — image, counts, vertex rows, boxes — to a second context built the same way and
    given the plain update of scene.skin_triangles of the caller's array; the second result is from the rest pose, not from the first."""
    from rvpt_amd import scene
    tris, mats, cam = cornell2
    rec = _skin.weights(tris, 7)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl, lab=True), native.Context(W, H, 0, 0, 1, fl, lab=True)
    try:
        assert a.build_scene(tris, mats, method=method) == b.build_scene(tris, mats, method=method)
        still = render(a, cam, 2)
        render(b, cam, 2)
        a.bind_skin(rec)
        results = []
        for phase in (0.0, 1.5):
            m = _skin.bones(tris, 7, phase)
            skinned = scene.skin_triangles(tris, rec, m)  # always from `tris`
            assert _skin.no_minus_zero(skinned)
            results.append(skinned)
            a.skin(m)
            b.update_triangles(skinned)
            got, want = render(a, cam, 2), render(b, cam, 2)
            assert not np.array_equal(bits(got), bits(still))
            assert np.array_equal(bits(got), bits(want)) and a.stats() == b.stats() and a.launch_info()[1:3] == b.launch_info()[1:3]
            sa, sb = a.scene_state(["tris", "nodes", "wide", "perm", "rest", "skin"]), b.scene_state(["tris", "nodes", "wide", "perm"])
            assert ds.same_bytes(sa["perm"], sb["perm"]) and ds.same_bytes(sa["tris"], sb["tris"]), ds.first_difference(sa["tris"], sb["tris"])
            assert ds.same_bytes(sa["tris"][:, :12], skinned[sa["perm"], :12])
            assert ds.same_nodes(sa["nodes"], sb["nodes"]) and ds.same_bytes(sa["wide"], sb["wide"])
            assert ds.same_bytes(sa["rest"], tris[sa["perm"], :12]) and sa["skin"].tobytes() == rec.tobytes()  # the binding stays in the caller's order
        assert results[0].tobytes() != results[1].tobytes()
        assert scene.skin_triangles(results[0], rec, _skin.bones(tris, 7, 1.5)).tobytes() != results[1].tobytes()  # (composing would have given another array)
    finally:
        a.close()
        b.close()


def test_a_mesh_larger_than_one_grid_of_work_groups(native):
    """skin_vertices runs on a grid the device holds at once — at most eight work-groups per CU, three where 1024 matrices fill 48 KiB of LDS each — and strides
    over the vertices.  67 712 triangles are 794 work-groups' worth with 1024 bones, more than three per CU on 256 CUs: some work-groups take a second round.
    The vertex rows against the statement, the boxes against a second context given the plain update."""
    from rvpt_amd import scene
    tris, mats = scene.heightfield_scene(184)
    n = tris.shape[0]
    assert n == 67712
    rng = np.random.RandomState(7)
    rec = np.zeros(3 * n, dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"] = rng.randint(0, 1024, size=(3 * n, 4))
    w = rng.uniform(0.1, 1.0, size=(3 * n, 4))
    rec["weight"] = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    rec["bone"][0, 0], rec["bone"][-1, 3] = 1023, 1023
    m = _skin.bones(tris, 1024)
    skinned = scene.skin_triangles(tris, rec, m)
    a, b = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True), native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        for ctx in (a, b):
            ctx.build_scene(tris, mats, method="lbvh")
        a.bind_skin(rec)
        a.skin(m)
        b.update_triangles(skinned)
        sa, sb = a.scene_state(["tris", "nodes", "wide", "perm"]), b.scene_state(["tris", "nodes", "wide", "perm"])
        assert ds.same_bytes(sa["perm"], sb["perm"]) and ds.same_bytes(sa["tris"][:, :12], skinned[sa["perm"], :12]), ds.first_difference(sa["tris"][:, :12], skinned[sa["perm"], :12])
        assert ds.same_bytes(sa["tris"], sb["tris"]) and ds.same_bytes(sa["nodes"], sb["nodes"]) and ds.same_bytes(sa["wide"], sb["wide"])
    finally:
        a.close()
        b.close()


# ---- the order of forms -----------------------------------------------------------------------------------------------------------------------------------------

def holds(ctx, nodes, want_tris, what):
    from rvpt_amd import scene
    s = ctx.scene_state(["tris", "nodes", "rest"])
    assert ds.same_bytes(s["tris"][:, :12], want_tris[:, :12]), (what, ds.first_difference(s["tris"][:, :12], want_tris[:, :12]))
    dev, _ = ds.device_layout(scene.refit_bvh(nodes, want_tris))
    assert ds.same_nodes(s["nodes"], dev), (what, "d_nodes")
    return s


def test_pose_and_sparse_updates_around_a_skin_update(native):
    """A pose update of one part after a skin update poses it from the rest pose and leaves the others skinned; a sparse update, then a skin update: the fresh
    snapshot includes the moved triangle; a plain full upload drops the binding and the next skin update is refused in the documented words."""
    from rvpt_amd import scene
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    rec, m, skinned = statement(tris, 3)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(nodes, tris, mats)
        ctx.bind_skin(rec)
        ctx.skin(m)
        s = holds(ctx, nodes, skinned, "skin")
        assert ds.same_bytes(s["rest"], tris[:, :12])
        moves = [(0, 63, about((0, 0, 2), rotation((0, 1, 0), 0.4)))]
        want = scene.pose_parts(tris, moves, current=skinned)
        assert _skin.no_minus_zero(want)
        ctx.pose_parts(moves)
        s = holds(ctx, nodes, want, "pose after skin: the part from the rest pose, the others stay skinned")
        assert ds.same_bytes(s["rest"], tris[:, :12])
        ctx.skin(m)
        holds(ctx, nodes, skinned, "skin after pose: every triangle again")
        # a sparse update ends the rest pose; the next skin update snapshots what the scene then holds
        row = skinned[100:101].copy()
        row[0, 0:12:4] += 0.125
        patched = skinned.copy()
        patched[100] = row[0]
        ctx.update_triangles(row, indices=np.array([100]))
        assert ctx.scene_state(["rest"])["rest"].size == 0 and ctx.scene_state(["skin"])["skin"].tobytes() == rec.tobytes()
        ctx.skin(m)
        again = scene.skin_triangles(patched, rec, m)
        s = holds(ctx, nodes, again, "skin, a sparse update, skin: the skinned and patched vertices are the new rest pose")
        assert ds.same_bytes(s["rest"], patched[:, :12]) and again.tobytes() != skinned.tobytes()
        # a plain and a guarded update keep the binding too
        ctx.update_triangles(np.ascontiguousarray(tris))
        ctx.update_triangles(np.ascontiguousarray(tris), rebuild_above=float("inf"))
        ctx.skin(m)
        holds(ctx, nodes, skinned, "plain update back, skin")
        img = render(ctx, cam, 2)
        # a full upload drops it
        ctx.upload_scene(nodes, tris, mats)
        assert ctx.scene_state(["skin"])["skin"].size == 0 and ctx.scene_state(["bones"])["bones"].size == 0
        with pytest.raises(native.NativeError, match="skin update before a bind") as e:
            ctx.skin(m)
        assert e.value.code == native.ERR_INVALID
        ctx.bind_skin(rec)
        ctx.skin(m)
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
    finally:
        ctx.close()


def test_a_guarded_pose_update_that_rebuilds_keeps_the_binding(native, cornell2):
    """skin, a guarded pose update that carries a part away and REBUILDS, skin with the same bones: the same vertices in the caller's order as before the
    rebuild — the binding is in the caller's order and goes through the new permutation, the rest pose went with the rebuild — and the frame of a fresh build of
    the posed triangles given the plain update of the skinned ones."""
    from rvpt_amd import scene
    tris, mats, cam = cornell2
    n = tris.shape[0]
    rec, m, skinned = statement(tris, 7)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl, lab=True), native.Context(W, H, 0, 0, 1, fl, lab=True)

    def callers_order(ctx):
        s = ctx.scene_state(["tris", "perm"])
        out = np.empty_like(s["tris"])
        out[s["perm"]] = s["tris"]
        return out, s["perm"]

    try:
        a.build_scene(tris, mats, method="lbvh")
        a.bind_skin(rec)
        a.skin(m)
        first, perm0 = callers_order(a)
        assert ds.same_bytes(first[:, :12], skinned[:, :12])
        away = [scene.part_move(0, 400, translation=(40.0, 30.0, 20.0))]
        report = a.pose_parts(away, rebuild_above=1.05)
        assert report.rebuilt and report.tree == "lbvh"
        posed, perm1 = callers_order(a)
        assert not np.array_equal(perm0, perm1) and ds.same_bytes(posed[:, :12], scene.pose_parts(tris, away, current=skinned)[:, :12])
        assert a.scene_state(["skin"])["skin"].tobytes() == rec.tobytes()
        a.skin(m)
        second, perm2 = callers_order(a)
        assert np.array_equal(perm1, perm2) and ds.same_bytes(second[:, :12], first[:, :12])
        b.build_scene(posed, mats, method="lbvh")
        b.update_triangles(skinned)
        got, want = render(a, cam, 2), render(b, cam, 2)
        assert np.array_equal(bits(got), bits(want)) and a.stats() == b.stats()
        sa, sb = a.scene_state(["tris", "nodes", "wide", "perm"]), b.scene_state(["tris", "nodes", "wide", "perm"])
        assert all(ds.same_bytes(sa[k], sb[k]) for k in ("tris", "wide", "perm")) and ds.same_nodes(sa["nodes"], sb["nodes"])
        # a build form the caller asks for drops the binding
        a.build_scene(tris, mats, method="lbvh")
        with pytest.raises(native.NativeError, match="skin update before a bind"):
            a.skin(m)
        assert n == 2300
    finally:
        a.close()
        b.close()


# ---- sources ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_weights_and_bones_from_device_tensors_give_the_host_arrays_bytes(native):
    import torch
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    rec, m, skinned = statement(tris, 3)
    a, b = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True), native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        for ctx in (a, b):
            ctx.upload_scene(nodes, tris, mats)
        a.bind_skin(rec)
        a.skin(m)
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1, 32).copy()).to("cuda:0")
        d_m = torch.from_numpy(m.copy()).to("cuda:0")
        b.bind_skin(d_rec)
        assert last_error(b) == ""
        b.skin(d_m)
        assert last_error(b) == ""
        sa, sb = a.scene_state(), b.scene_state()
        for k in ("tris", "nodes", "wide", "rest", "skin", "bones"):
            assert ds.same_bytes(sa[k], sb[k]), k
        assert ds.same_bytes(sb["tris"][:, :12], skinned[:, :12]) and sb["bones"].tobytes() == m.tobytes()
        assert np.array_equal(bits(render(a, cam, 2)), bits(render(b, cam, 2)))
        # int32 / float32 views of the same records and [k, 12] matrices are the same memory
        b.bind_skin(d_rec.view(torch.int32))
        b.skin(d_m.reshape(-1, 12))
        assert ds.same_bytes(b.scene_state(["tris"])["tris"], sa["tris"])
        if torch.cuda.device_count() > 1:  # another GPU's memory is refused, naming both devices
            other = d_m.to("cuda:1")
            with pytest.raises(native.NativeError, match="device 1, the context on 0"):
                b.skin(other)
            rc = b._L.rvpt_hip_upload_scene(b._h, ctypes.c_void_p(other.data_ptr()), native.NODES_UPDATE_SKIN, None, 3, None, 0)
            assert rc == native.ERR_INVALID and "device memory of GPU 1, the context lives on GPU 0" in last_error(b)
            o_rec = d_rec.to("cuda:1")
            rc = b._L.rvpt_hip_upload_scene(b._h, ctypes.c_void_p(o_rec.data_ptr()), native.NODES_BIND_SKIN, None, tris.shape[0], None, 0)
            assert rc == native.ERR_INVALID and "device memory of GPU 1, the context lives on GPU 0" in last_error(b)
            assert ds.same_bytes(b.scene_state(["tris"])["tris"], sa["tris"])
    finally:
        a.close()
        b.close()


# ---- read-back --------------------------------------------------------------------------------------------------------------------------------------------------

def test_read_back_after_bind_and_after_skin(native):
    """the laboratory build's pieces against the numpy statements byte for byte: TRIS vertex rows, NODES boxes, WIDE, REST, SKIN in update order, BONES"""
    import torch
    from rvpt_amd import scene
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    n = tris.shape[0]
    rec, m, skinned = statement(tris, 1024)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(nodes, tris, mats)
        s0 = ctx.scene_state()
        assert s0["skin"].size == 0 and s0["bones"].size == 0 and s0["rest"].size == 0 and s0["n_wide"] > 0
        ctx.bind_skin(rec)
        s1 = ctx.scene_state()
        assert s1["skin"].shape == (3 * n,) and s1["skin"].dtype == native.VERTEX_SKIN_DTYPE and s1["skin"].tobytes() == rec.tobytes()
        assert s1["bones"].size == 0 and s1["rest"].size == 0  # a bind takes no snapshot and ends none
        for k in ("tris", "nodes", "wide", "wide_map", "refit_levels", "perm"):
            assert ds.same_bytes(s0[k], s1[k]), k
        ctx.skin(torch.from_numpy(m.copy()).to("cuda:0"))
        s2 = ctx.scene_state()
        want_nodes = scene.refit_bvh(s0["nodes"], skinned).view(native.NODE_DTYPE).reshape(-1)
        assert ds.same_bytes(s2["tris"][:, :12], skinned[:, :12]), ds.first_difference(s2["tris"][:, :12], skinned[:, :12])
        assert ds.same_bytes(s2["tris"][:, 12:], s0["tris"][:, 12:])
        assert ds.same_nodes(s2["nodes"], want_nodes), ds.first_difference(s2["nodes"], want_nodes)
        assert ds.same_bytes(s2["wide"], ds.regathered(s0["wide"], s0["wide_map"], want_nodes))
        assert s2["rest"].shape == (n, 12) and ds.same_bytes(s2["rest"], tris[:, :12])
        assert s2["skin"].tobytes() == rec.tobytes() and s2["bones"].shape == (1024, 12) and s2["bones"].tobytes() == m.tobytes()
        for k in ("wide_map", "refit_levels", "perm", "n_tris", "n_nodes", "n_wide", "bvh_height", "bvh_head_shift", "wide_stack_levels", "built_by", "have_perm", "base_cost"):
            assert ds.same_bytes(s0[k], s2[k]) if isinstance(s0[k], np.ndarray) else s0[k] == s2[k], k
        # a second skin update: from the same rest pose, which it leaves as it was
        m2 = _skin.bones(tris, 1024, phase=0.8)
        ctx.skin(m2)
        s3 = ctx.scene_state(["tris", "rest", "bones"])
        assert ds.same_bytes(s3["rest"], s2["rest"]) and ds.same_bytes(s3["tris"][:, :12], scene.skin_triangles(tris, rec, m2)[:, :12]) and s3["bones"].tobytes() == m2.tobytes()
        # a second bind replaces the first
        rec2 = _skin.weights(tris, 3)
        ctx.bind_skin(rec2)
        s4 = ctx.scene_state(["skin", "bones", "rest", "tris"])
        assert s4["skin"].tobytes() == rec2.tobytes() and s4["bones"].size == 0 and ds.same_bytes(s4["rest"], s2["rest"]) and ds.same_bytes(s4["tris"], s3["tris"])
        ctx.skin(m2[:3])
        assert ds.same_bytes(ctx.scene_state(["tris"])["tris"][:, :12], scene.skin_triangles(tris, rec2, m2[:3])[:, :12])
    finally:
        ctx.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------------

def raw(native, ctx, count, lst, n, tris=None, mats=None, offset=0):
    """the C call itself: (return code, message); lst: a numpy array, a device pointer (int) or None"""
    keep = np.ascontiguousarray(lst) if isinstance(lst, np.ndarray) else None
    ptr = None if lst is None else ctypes.c_void_p((keep.ctypes.data if keep is not None else int(lst)) + offset)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=np.float32)
    mm = None if mats is None else np.ascontiguousarray(mats, dtype=np.float32)
    rc = ctx._L.rvpt_hip_upload_scene(ctx._h, ptr, count, None if t is None else t.ctypes.data_as(ctypes.c_void_p), n, None if mm is None else mm.ctypes.data_as(ctypes.c_void_p),
                                      0 if mm is None else mm.shape[0])
    return rc, last_error(ctx)


def test_refusals_in_order_leave_everything_as_it_was(native):
    """Every case offends at its own place in the documented order AND at every later place it can be combined with: the message is the earlier one's."""
    import torch
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    n = tris.shape[0]
    rec, m, skinned = statement(tris, 7)
    BIND, SKIN = native.NODES_BIND_SKIN, native.NODES_UPDATE_SKIN
    bad = rec.copy()
    bad["bone"][70, 1], bad["bone"][50, 2], bad["bone"][50, 3] = 5000, 1024, 9999
    top = int(rec["bone"].max())
    top_pos = int(np.argwhere(rec["bone"] == top)[0][0])
    assert top == 6
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        assert raw(native, ctx, BIND, None, n + 1) == (native.ERR_INVALID, "bind before any full upload_scene on this context: there is no scene to bind weights to")
        rc, msg = raw(native, ctx, SKIN, None, 0)
        assert rc == native.ERR_INVALID and "skin update before any full upload_scene" in msg
        ctx.upload_scene(nodes, tris, mats)
        rc, msg = raw(native, ctx, SKIN, m, 7)
        assert rc == native.ERR_INVALID and "skin update before a bind" in msg
        ctx.bind_skin(rec)
        ctx.skin(m)
        img = render(ctx, cam, 2)
        s0 = ctx.scene_state(["tris", "nodes", "rest", "wide", "skin", "bones"])
        assert ds.same_bytes(s0["tris"][:, :12], skinned[:, :12])

        def untouched(what):
            s = ctx.scene_state(["tris", "nodes", "rest", "wide", "skin", "bones"])
            for k in s0:
                assert ds.same_bytes(s[k], s0[k]), (what, k)
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img)), what

        d_bad = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        d_rec = torch.from_numpy(np.concatenate([np.zeros(4, np.uint8), rec.view(np.uint8).reshape(-1)])).to("cuda:0")  # the records at an offset of four bytes
        d_m = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), m.reshape(-1)])).to("cuda:0")
        assert d_bad.data_ptr() % 16 == 0 and d_rec.data_ptr() % 16 == 0 and d_m.data_ptr() % 16 == 0
        two = np.concatenate([bad, bad])
        bind_cases = [((None, n + 1), f"bind for {n + 1} triangles, the uploaded scene has {n}"),
                      ((None, n, tris[:1]), "bind without a list"),
                      ((two, n, tris[:1], None, 2), "is not 4-byte aligned"),
                      ((d_rec.data_ptr() + 4, n, tris[:1]), "is not 16-byte aligned"),
                      ((bad, n, tris[:1], mats), "bind takes no triangles"),
                      ((bad, n, None, mats), "bind takes no materials"),
                      ((bad, n), f"bind: skin[50].bone[2] = 1024: a bone index lies below 1024"),
                      ((d_bad.data_ptr(), n), f"bind: skin[50].bone[2] = 1024: a bone index lies below 1024")]
        for args, what in bind_cases:
            rc, msg = raw(native, ctx, BIND, *args)
            assert rc == native.ERR_INVALID and what in msg, (what, rc, msg)
            untouched(what)
        big = np.zeros((1025, 12), dtype=np.float32)
        skin_cases = [((None, 0, tris[:1]), "skin update without bones"),
                      ((None, 1025, tris[:1]), "skin update with 1025 bones: at most 1024"),
                      ((None, 6, tris[:1]), "skin update without a list"),
                      ((big, 6, tris[:1], None, 2), "is not 4-byte aligned"),
                      ((d_m.data_ptr() + 4, 6, tris[:1]), "is not 16-byte aligned"),
                      ((m, 6, tris[:1], mats), "skin update takes no triangles"),
                      ((m, 6, None, mats), "skin update takes no materials"),
                      ((m, 6), f"skin update with 6 bones: the binding names bone 6 (skin[{top_pos}]), which needs 7"),
                      ((d_m.data_ptr() + 16, 6), f"skin update with 6 bones: the binding names bone 6 (skin[{top_pos}]), which needs 7")]
        for args, what in skin_cases:
            rc, msg = raw(native, ctx, SKIN, *args)
            assert rc == native.ERR_INVALID and what in msg, (what, rc, msg)
            untouched(what)
        # through the wrappers the library's words arrive as they are
        with pytest.raises(native.NativeError, match=r"skin\[50\]\.bone\[2\] = 1024") as e:
            ctx.bind_skin(bad)
        assert e.value.code == native.ERR_INVALID
        with pytest.raises(native.NativeError, match="the binding names bone 6"):
            ctx.skin(m[:6])
        untouched("wrappers")
        # the same calls with good lists are the bind and the update, and leave no message; the device list of 1023 is legal
        ok = rec.copy()
        ok["bone"][5, 3] = 1023
        d_ok = torch.from_numpy(ok.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        assert raw(native, ctx, BIND, d_ok.data_ptr(), n) == (0, "")
        rc, msg = raw(native, ctx, SKIN, np.zeros((1023, 12), np.float32), 1023)
        assert rc == native.ERR_INVALID and "the binding names bone 1023 (skin[5]), which needs 1024" in msg
        assert raw(native, ctx, BIND, rec, n) == (0, "") and raw(native, ctx, SKIN, m.reshape(-1, 12), 7) == (0, "")
        untouched("the same bind and the same bones again")
    finally:
        ctx.close()


def test_caller_layout_has_no_skin_form(native, monkeypatch):
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    rec, m, _ = statement(tris, 3)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(nodes, tris, mats)
        img = render(ctx, cam, 1)
        with pytest.raises(native.NativeError, match="skin update before a bind"):  # (the earlier refusal)
            ctx.skin(m)
        ctx.bind_skin(rec)
        with pytest.raises(native.NativeError, match="CALLER_LAYOUT") as e:
            ctx.skin(m)
        assert e.value.code == native.ERR_UNSUPPORTED
        with pytest.raises(native.NativeError, match="CALLER_LAYOUT"):  # the plain form's answer
            ctx.update_triangles(np.ascontiguousarray(tris))
        assert np.array_equal(bits(render(ctx, cam, 1)), bits(img)) and ctx.scene_state(["rest"])["rest"].size == 0
    finally:
        ctx.close()


# ---- brute-force contexts ---------------------------------------------------------------------------------------------------------------------------------------

def test_brute_force_context(native):
    """bind + skin equals the plain update with scene.skin_triangles' array; the binding and the rest pose live on the host; a device pointer is refused"""
    import torch
    from rvpt_amd import scene
    (tris, mats, _), cam = scene_and_camera("default", W, H)
    n = tris.shape[0]
    rec = _skin.weights(tris, 3)
    a, b = native.Context(W, H, 0, 0, 1, native.COUNT_SEGMENTS, lab=True), native.Context(W, H, 0, 0, 1, native.COUNT_SEGMENTS, lab=True)
    try:
        for ctx in (a, b):
            ctx.upload_scene(None, tris, mats)
        still = render(a, cam, 2)
        render(b, cam, 2)
        a.bind_skin(rec)
        assert np.array_equal(bits(render(a, cam, 2)), bits(still))
        render(b, cam, 2)
        for phase in (0.0, 1.1):
            m = _skin.bones(tris, 3, phase)
            skinned = scene.skin_triangles(tris, rec, m)
            a.skin(m)
            assert last_error(a) == ""
            b.update_triangles(skinned)
            got, want = render(a, cam, 2), render(b, cam, 2)
            assert not np.array_equal(bits(got), bits(still)) and np.array_equal(bits(got), bits(want))
            assert a.stats() == b.stats() and a.launch_info() == b.launch_info() and a.cull_info() == b.cull_info()
            s = a.scene_state(["tris", "rest", "skin", "bones"])
            assert ds.same_bytes(s["tris"][:, :12], skinned[:, :12]) and ds.same_bytes(s["rest"], tris[:, :12]) and s["skin"].tobytes() == rec.tobytes() and s["bones"].size == 0
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        d_m = torch.from_numpy(m.copy()).to("cuda:0")
        rc, msg = raw(native, a, native.NODES_BIND_SKIN, d_rec.data_ptr(), n)
        assert rc == native.ERR_INVALID and "bind on a brute-force context from a device pointer" in msg
        rc, msg = raw(native, a, native.NODES_UPDATE_SKIN, d_m.data_ptr(), 3)
        assert rc == native.ERR_INVALID and "skin update of a brute-force context from a device pointer" in msg
        assert np.array_equal(bits(render(a, cam, 2)), bits(got))
        a.pose_parts([(0, 63, about((0, 0, 2), rotation((0, 1, 0), 0.4)))])  # from the shared rest pose, the others stay skinned
        want = scene.pose_parts(tris, [(0, 63, about((0, 0, 2), rotation((0, 1, 0), 0.4)))], current=skinned)
        assert ds.same_bytes(a.scene_state(["tris"])["tris"][:, :12], want[:, :12])
    finally:
        a.close()
        b.close()


# ---- queries ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_ray_queries_answer_on_the_skinned_scene(native, oracle):
    from rvpt_amd import scene
    (tris, mats, nodes), _ = scene_and_camera("default", W, H)
    rec, m, skinned = statement(tris, 7)
    refit = scene.refit_bvh(nodes, skinned)
    records = rq.poisoned(rq.base_rays(skinned, 11, counts=(20, 20, 10, 10, 10, 10)))
    want = rq.Statement(oracle, refit, skinned).answer(records, 0)
    still = rq.Statement(oracle, nodes, tris).answer(records, 0)
    assert not rq.same_bytes(want, still) and 10 < int((want["prim"] != rq.NO_PRIM).sum())
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, tris, mats)
        ctx.bind_skin(rec)
        ctx.skin(m)
        got = ctx.trace_rays_into(records.copy())
        assert rq.same_bytes(got, want), rq.first_difference(got, want)  # prim numbered as before: the stored order
    finally:
        ctx.close()


# ---- the RVPT mirror --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", ["host", "device-sah"])
def test_renderer_mirror(native, build):
    """RVPT.bind_skin takes the records of the triangles in the order they were ADDED: the frame after RVPT.skin equals that of update_triangles(
    scene.skin_triangles(...)) on a second object, the mirror's host copies follow, and bvh_nodes is the refit of the tree as built."""
    from rvpt_amd import RVPT, scene
    tris, mats = scene.default_scene()
    rec = _skin.weights(tris, 7)
    pair = []
    for _ in range(2):
        r = RVPT(W, H, device=0, traversal="bvh", build=build)
        r.add_triangles(tris)
        for mat in mats:
            r.add_material(mat)
        r.initialize()
        pair.append(r)
    a, b = pair

    def frames():
        out = []
        for r in pair:
            r.update()
            assert r.render_settings.current_frame == 0
            r.draw()
            r.update()
            r.draw()
            out.append(r.read_frame())
        return out

    try:
        built, order = a.bvh_nodes.copy(), np.asarray(a.primitive_indices).astype(np.int64)
        still = frames()[0]
        a.bind_skin(rec)
        for phase in (0.0, 0.9):
            m = _skin.bones(tris, 7, phase)
            skinned = scene.skin_triangles(tris, rec, m)
            assert a.skin(m) is None
            b.update_triangles(skinned)
            got, want = frames()
            assert not np.array_equal(bits(got), bits(still)) and np.array_equal(bits(got), bits(want))
            assert np.array_equal(np.concatenate(a.triangles), skinned) and np.array_equal(a.sorted_triangles, skinned[order])
            assert a.bvh_nodes.tobytes() == scene.refit_bvh(built, skinned[order]).tobytes() == b.bvh_nodes.tobytes()
    finally:
        a.shutdown()
        b.shutdown()
