"""The pose update on the GPU: rvpt_hip_upload_scene's RVPT_HIP_NODES_UPDATE_POSE form (Context.pose_parts) moves ranges of triangles by one 3x4 matrix each,
posed on the device from the rest pose it keeps, and refits only the paths above them.  Everything here is bit-exact: after an update the context renders what a
fresh context given upload_scene(refit_bvh(nodes, posed, touched), posed, mats) renders and what the CPU oracle renders on that tree, with
posed = scene.pose_parts(...), and the laboratory build's read-back shows the same bytes the numpy statements give.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import _device_state as ds
import _ray_query as rq
from _util import identity_camera, scene_by_name
from test_gpu_parity import oracle_frames
from test_pose_host import about, rotation
from test_refit import bits, flags_of, render, scene_and_camera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


@pytest.fixture(scope="module")
def cornell600():
    """cornell_scene at the smallest subdivision with at least 600 triangles (2: 2300, nine work-groups of pose_parts), in leaf order, with its camera"""
    from rvpt_amd import Camera, native as nat, scene
    assert scene.cornell_scene(1)[0].shape[0] < 600
    tris, mats = scene.cornell_scene(2)
    assert tris.shape[0] >= 600
    nodes, idx = nat.build_bvh(tris)
    c = Camera(64 / 48)
    c.translation = np.array([0.0, 2.0, -1.9])
    tris = tris[idx]
    for a in (tris, mats, nodes):
        a.setflags(write=False)
    return tris, mats, nodes, c.get_data()


def centroid(tris, first, count):
    return tris[first:first + count].reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64).mean(axis=0)


def listed_of(moves):
    from rvpt_amd import scene
    rec = scene.part_moves(moves)
    return np.concatenate([np.arange(int(r["first"]), int(r["first"]) + int(r["count"]), dtype=np.int64) for r in rec])


def no_minus_zero(tris) -> bool:
    """min / max of floats, hence byte equality of boxes, is well defined where no coordinate is -0 beside a +0; the scenes here hold no -0 and the pose
    arithmetic makes none (a sum that cancels is +0)"""
    v = ds.vertices(tris)
    return not bool(((v == 0) & np.signbit(v)).any())


SCALE_SHEAR = np.array([[1.2, 0.25, 0.0, 0.05], [0.0, 0.5, 0.2, -0.1], [0.1, 0.0, 1.1, 0.2]])  # (brings the upper part of the default model into the identity camera's view)


def three_updates(tris):
    """the three pose updates of the default scene's parts [0, 63), [63, 64), [64, 143): a rotation about a part's centroid; a translation and a non-uniform
    scale with shear at once; the first part again with another rotation (from the rest pose) and the one-triangle part by another translation"""
    from rvpt_amd import scene
    n = tris.shape[0]
    c0 = centroid(tris, 0, 63)
    return [[(0, 63, about(c0, rotation((0.2, 1, 0.1), 0.5)))],
            [scene.part_move(63, 1, translation=(0.15, 0.2, -0.1)), (64, n - 64, SCALE_SHEAR)],
            [(0, 63, about(c0, rotation((1, 0.3, 0), -0.4))), scene.part_move(63, 1, translation=(-0.2, 0.1, 0.0))]]


def fresh(native, fl, W, H, nodes, tris, mats, cam, aa=1, batch=False, lab=None):
    ctx = native.Context(W, H, 0, 0, 1, fl, lab=lab)
    try:
        ctx.upload_scene(nodes, tris, mats)
        return render(ctx, cam, 2, aa=aa, batch=batch), ctx.stats(), ctx.launch_info()
    finally:
        ctx.close()


# ---- 1. renders as a fresh upload ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("traversal,knob", [("bvh", None), ("bvh_ordered", None), ("bvh", "RVPT_HIP_BVH_NO_RESIDENT")])
def test_three_pose_updates_render_as_fresh_uploads_of_the_refit_tree(native, oracle, monkeypatch, traversal, knob, batch):
    from rvpt_amd import scene
    W, H = 64, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    assert tris.shape[0] == 143 and no_minus_zero(tris)
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
        if knob:
            assert info[2] == 10
        elif traversal == "bvh":
            assert info[2] == 11
        posed, current = tris, nodes
        for moves in three_updates(tris):
            posed = scene.pose_parts(tris, moves, current=posed)
            assert no_minus_zero(posed)
            current = scene.refit_bvh(current, posed, touched=listed_of(moves))
            assert current.tobytes() == scene.refit_bvh(nodes, posed).tobytes()  # (a tight tree: the sparse refit is the full one)
            ctx.pose_parts(moves)
            got = render(ctx, cam, 2, batch=batch)
            now = ctx.stats()
            want, want_stats, want_info = fresh(native, fl, W, H, current, posed, mats, cam, batch=batch, lab=lab)
            ref, seg = oracle_frames(oracle, (posed, mats, current), cam, W, H, traversal, [0, 1])
            assert not np.array_equal(bits(got), bits(before)), "the geometry did not move"
            assert np.array_equal(bits(got), bits(want)), "pose update != fresh upload of the refit tree"
            assert np.array_equal(bits(got), bits(ref[1])), "pose update != oracle"
            assert (now[0] - seen[0], now[1] - seen[1]) == want_stats and want_stats[0] == seg
            # the kernel path is the fresh upload's; the LDS bytes stay the context's own: they follow the grouping of the wide form, which an update keeps
            # from the upload and which a fresh upload of a tree moved this far may make anew (tests/test_device_state.py: check_update_state)
            assert ctx.launch_info()[2] == info[2] == want_info[2] and ctx.launch_info()[1] == info[1]
            seen, before = now, got
    finally:
        ctx.close()


def test_showcase_scene_with_one_part(native, oracle):
    """mirror, glass and emitter: one part of the showcase scene rotated about its centroid"""
    from rvpt_amd import scene
    W, H = 64, 48
    tris, mats, nodes = scene_by_name("showcase")
    cam = identity_camera(W / H)
    moves = [(40, 60, about(centroid(tris, 40, 60), rotation((0, 1, 0), 0.6)))]
    posed = scene.pose_parts(tris, moves)
    refit = scene.refit_bvh(nodes, posed, touched=listed_of(moves))
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes, tris, mats)
        before = render(ctx, cam, 2)
        seen = ctx.stats()
        ctx.pose_parts(moves)
        got = render(ctx, cam, 2)
        now = ctx.stats()
    finally:
        ctx.close()
    want, want_stats, _ = fresh(native, fl, W, H, refit, posed, mats, cam)
    ref, seg = oracle_frames(oracle, (posed, mats, refit), cam, W, H, "bvh", [0, 1])
    assert not np.array_equal(bits(got), bits(before))
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(ref[1]))
    assert (now[0] - seen[0], now[1] - seen[1]) == want_stats and want_stats[0] == seg


# ---- 2 and 9. ranges at the edges the kernel can get wrong, with the device state ---------------------------------------------------------------------------------

def edge_moves(name, tris, nodes):
    from rvpt_amd import native as nat, scene
    n = tris.shape[0]
    turn = about(centroid(tris, 0, n), rotation((0.1, 1, 0.2), 0.3))
    lift = scene.part_move(0, 1, translation=(0.05, 0.12, -0.07))["m"].reshape(3, 4)
    if name == "inside_a_leaf":  # the leaf then holds posed and unposed triangles
        rec = np.ascontiguousarray(nodes).view(nat.NODE_DTYPE).reshape(-1)
        leaf = int(np.argmax(rec["count"]))  # the largest leaf: the range leaves out its first triangle and, where it holds three or more, its last
        assert rec["count"][leaf] >= 2
        return [(int(rec["first"][leaf]) + 1, max(1, int(rec["count"][leaf]) - 2), lift)]
    if name == "one_triangle":
        return [(n // 2, 1, turn)]
    if name == "across_a_work_group":  # threads 0 .. 256: five waves, two work-groups, triangles 63 .. 319
        return [(63, 257, turn)]
    if name == "two_parts_meet_in_a_wave":  # thread 96 = lane 32 of the second wave is the first of the second part
        return [(10, 96, turn), (106, 150, lift)]
    if name == "second_part_listed_first":  # the same ranges, the list the other way round: the prefix sums follow the LIST, not the positions
        return [(106, 150, lift), (10, 96, turn)]
    if name == "whole_scene":
        return [(0, n, turn)]
    assert name == "every_triangle_a_part"
    out = np.zeros(n, dtype=nat.PART_MOVE_DTYPE)
    out["first"], out["count"] = np.arange(n), 1
    m = np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1))
    m[:, :, 3] = 0.05 * np.sin(np.arange(n)[:, None] * np.array([0.31, 0.17, 0.23]) + np.array([0.0, 1.0, 2.0]))
    m[:, 0, 1] = 0.1 * np.cos(0.05 * np.arange(n))  # a shear of its own per triangle
    out["m"] = m.reshape(n, 12)
    return out


EDGES = ["inside_a_leaf", "one_triangle", "across_a_work_group", "two_parts_meet_in_a_wave", "second_part_listed_first", "whole_scene", "every_triangle_a_part"]


@pytest.mark.parametrize("name", EDGES)
def test_edge_ranges_image_and_device_state(native, cornell600, name):
    """after the update: the image of a fresh upload of the statement, and in the laboratory build's read-back TRIS = scene.pose_parts, NODES = refit_bvh(touched=),
    WIDE = the upload's wide form with those boxes, no flag left set, REST = the vertices before the pose; REST is gone after a plain update"""
    from rvpt_amd import scene
    W, H = 64, 48
    tris, mats, nodes, cam = cornell600
    n = tris.shape[0]
    moves = edge_moves(name, tris, nodes)
    listed = listed_of(moves)
    posed = scene.pose_parts(tris, moves)
    assert no_minus_zero(tris) and no_minus_zero(posed) and not np.array_equal(bits(posed[listed, :12]), bits(tris[listed, :12]))
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(W, H, 0, 0, 1, fl, lab=True)
    try:
        ctx.upload_scene(nodes, tris, mats)
        s0 = ctx.scene_state()
        assert s0["rest"].size == 0 and s0["n_wide"] > 0
        before = render(ctx, cam, 2)
        seen = ctx.stats()
        ctx.pose_parts(moves)
        assert ctx._L.rvpt_hip_last_error(ctx._h) in (None, b"")
        s1 = ctx.scene_state()
        got = render(ctx, cam, 2)
        now = ctx.stats()
        want_nodes = scene.refit_bvh(s0["nodes"], posed, touched=listed).view(native.NODE_DTYPE).reshape(-1)
        assert ds.same_bytes(s1["tris"][:, :12], posed[:, :12]), ("d_tris bytes 0-47", ds.first_difference(s1["tris"][:, :12], posed[:, :12]))
        assert ds.same_bytes(s1["tris"][:, 12:], s0["tris"][:, 12:])
        assert ds.same_nodes(s1["nodes"], want_nodes), ("d_nodes", ds.first_difference(s1["nodes"], want_nodes))
        assert ds.same_bytes(s1["wide"], ds.regathered(s0["wide"], s0["wide_map"], want_nodes))
        assert s1["have_sparse_maps"] and s1["sparse_dirty"].size > 0 and not s1["sparse_dirty"].any()
        assert s1["rest"].shape == (n, 12) and ds.same_bytes(s1["rest"], tris[:, :12])
        for k in ("wide_map", "refit_levels", "perm", "n_tris", "n_nodes", "n_wide", "bvh_height", "bvh_head_shift", "wide_stack_levels", "built_by", "have_perm", "base_cost"):
            assert ds.same_bytes(s0[k], s1[k]) if isinstance(s0[k], np.ndarray) else s0[k] == s1[k], k
        # the same list again: from the rest pose, so nothing moves, and the snapshot is the one taken before
        ctx.pose_parts(moves)
        s2 = ctx.scene_state(["tris", "nodes", "rest", "sparse_dirty"])
        assert ds.same_bytes(s2["tris"], s1["tris"]) and ds.same_nodes(s2["nodes"], s1["nodes"]) and ds.same_bytes(s2["rest"], s1["rest"]) and not s2["sparse_dirty"].any()
        ctx.update_triangles(np.ascontiguousarray(tris))
        assert ctx.scene_state(["rest"])["rest"].size == 0
    finally:
        ctx.close()
    caller_nodes = scene.refit_bvh(nodes, posed, touched=listed)
    want, want_stats, want_info = fresh(native, fl, W, H, caller_nodes, posed, mats, cam, lab=True)
    if listed.size > 1:  # (one triangle out of 2300 need not be in view)
        assert not np.array_equal(bits(got), bits(before))
    assert np.array_equal(bits(got), bits(want)) and (now[0] - seen[0], now[1] - seen[1]) == want_stats


# ---- 3. semantics ---------------------------------------------------------------------------------------------------------------------------------------------

def test_semantics_of_the_rest_pose(native):
    """B after A of the same part is B alone; B of another part leaves the first at A; a sparse update in between makes the A-posed vertices the new rest pose; a
    plain update back to the original triangles, then the same pose, gives the first time's bytes"""
    from rvpt_amd import scene
    (tris, mats, nodes), _ = scene_and_camera("default", 64, 48)
    n = tris.shape[0]
    A = [(0, 63, about(centroid(tris, 0, 63), rotation((0, 1, 0), 0.4)))]
    B = [(0, 63, about(centroid(tris, 0, 63), rotation((1, 0, 0), -0.3)))]
    B2 = [(64, n - 64, SCALE_SHEAR)]
    ctx = native.Context(64, 48, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)

    def holds(want_tris, what):
        s = ctx.scene_state(["tris", "nodes"])
        assert ds.same_bytes(s["tris"][:, :12], want_tris[:, :12]), (what, ds.first_difference(s["tris"][:, :12], want_tris[:, :12]))
        dev, _ = ds.device_layout(scene.refit_bvh(nodes, want_tris))  # (a tight tree: every sparse refit is the full one)
        assert ds.same_nodes(s["nodes"], dev), (what, "d_nodes")
        return s

    try:
        ctx.upload_scene(nodes, tris, mats)
        ctx.pose_parts(A)
        after_a = scene.pose_parts(tris, A)
        first_time = holds(after_a, "A")
        ctx.pose_parts(B)
        holds(scene.pose_parts(tris, B), "A then B of the same part = B alone")
        assert scene.pose_parts(tris, B).tobytes() != scene.pose_parts(after_a, B).tobytes()
        ctx.pose_parts(A)
        ctx.pose_parts(B2)
        holds(scene.pose_parts(tris, B2, current=after_a), "A of part 1 then B of part 2: part 1 stays at A")
        # the snapshot rule
        ctx.upload_scene(nodes, tris, mats)
        ctx.pose_parts(A)
        row = after_a[100:101].copy()
        row[0, 0:12:4] += 0.125
        patched = after_a.copy()
        patched[100] = row[0]
        ctx.update_triangles(row, indices=np.array([100]))
        assert ctx.scene_state(["rest"])["rest"].size == 0
        ctx.pose_parts(B)
        holds(scene.pose_parts(patched, B), "A, a sparse update, B: B applied to the A-posed vertices")
        assert ds.same_bytes(ctx.scene_state(["rest"])["rest"], patched[:, :12])
        # back to the original triangles by the plain form, then the same pose
        ctx.update_triangles(np.ascontiguousarray(tris))
        ctx.pose_parts(A)
        again = holds(after_a, "pose, plain update back, the same pose")
        assert ds.same_bytes(again["tris"], first_time["tris"]) and ds.same_bytes(again["nodes"], first_time["nodes"])
        # an empty list changes nothing, whatever its form
        ctx.pose_parts([])
        ctx.pose_parts(np.zeros(0, dtype=native.PART_MOVE_DTYPE))
        holds(after_a, "an empty list")
    finally:
        ctx.close()


# ---- 4. after each build form -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_after_build_scene_ranges_are_in_the_callers_order(native, cornell600, method):
    """After a build form the ranges number the triangles as the caller passed them: equal — image, counts, vertex rows and boxes — to a second context built the
    same way and given the plain update of scene.pose_parts of the caller's array."""
    from rvpt_amd import scene
    W, H = 64, 48
    sorted_tris, mats, _, cam = cornell600
    rng = np.random.RandomState(17)
    tris = sorted_tris[rng.permutation(sorted_tris.shape[0])]  # the caller's order: any order
    n = tris.shape[0]
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl, lab=True), native.Context(W, H, 0, 0, 1, fl, lab=True)
    try:
        assert a.build_scene(tris, mats, method=method) == b.build_scene(tris, mats, method=method)
        still = render(a, cam, 2)
        render(b, cam, 2)
        posed = tris
        for moves in ([(63, 257, about(centroid(tris, 63, 257), rotation((0, 1, 0), 0.4)))],
                      [(63, 257, about(centroid(tris, 63, 257), rotation((1, 0, 0), 0.2))), (400, n - 400, SCALE_SHEAR), scene.part_move(0, 1, translation=(0.1, 0.1, 0.1))]):
            posed = scene.pose_parts(tris, moves, current=posed)
            a.pose_parts(moves)
            b.update_triangles(posed)
            got, want = render(a, cam, 2), render(b, cam, 2)
            assert not np.array_equal(bits(got), bits(still))
            assert np.array_equal(bits(got), bits(want)) and a.stats() == b.stats() and a.launch_info()[1:3] == b.launch_info()[1:3]
            sa, sb = a.scene_state(["tris", "nodes", "wide", "perm", "rest"]), b.scene_state(["tris", "nodes", "wide", "perm"])
            assert ds.same_bytes(sa["perm"], sb["perm"]) and ds.same_bytes(sa["tris"], sb["tris"]) and ds.same_bytes(sa["tris"][:, :12], posed[sa["perm"], :12])
            assert ds.same_nodes(sa["nodes"], sb["nodes"]) and ds.same_bytes(sa["wide"], sb["wide"])  # (a built tree is tight: the paths' refit is the full one)
            assert ds.same_bytes(sa["rest"], tris[sa["perm"], :12])
        # a rebuild replaces the permutation and the scene: the inverse and the rest pose the library kept must not survive it
        again = posed[rng.permutation(n)]
        a.build_scene(again, mats, method=method)
        b.build_scene(again, mats, method=method)
        moves = [(5, 300, about(centroid(again, 5, 300), rotation((0, 0, 1), 0.3)))]
        a.pose_parts(moves)
        b.update_triangles(scene.pose_parts(again, moves))
        assert np.array_equal(bits(render(a, cam, 2)), bits(render(b, cam, 2)))
        sa = a.scene_state(["perm", "rest"])
        assert ds.same_bytes(sa["rest"], again[sa["perm"], :12])
    finally:
        a.close()
        b.close()


# ---- 5. brute-force contexts ------------------------------------------------------------------------------------------------------------------------------------

def test_brute_force_context(native):
    """The culls on: the image, the counts and the culls of a fresh brute-force upload of the posed triangles; the rest pose lives on the host and follows the
    same rules."""
    from rvpt_amd import scene
    W, H = 160, 96  # (the size at which the sparse update's brute-force case rides the packet kernel with every cull)
    (tris, mats, _), cam = scene_and_camera("default", W, H)
    updates = three_updates(tris)
    a = native.Context(W, H, 0, 0, 1, native.COUNT_SEGMENTS, lab=True)
    try:
        a.upload_scene(None, tris, mats)
        still = render(a, cam, 2, aa=2)
        assert a.scene_state(["rest"])["rest"].size == 0
        posed = tris
        for moves in updates:
            posed = scene.pose_parts(tris, moves, current=posed)
            seen = a.stats()
            a.pose_parts(moves)
            assert a._L.rvpt_hip_last_error(a._h) in (None, b"")
            got = render(a, cam, 2, aa=2)
            now = a.stats()
            b = native.Context(W, H, 0, 0, 1, native.COUNT_SEGMENTS, lab=True)
            try:
                b.upload_scene(None, posed, mats)
                want = render(b, cam, 2, aa=2)
                assert np.array_equal(bits(got), bits(want)) and (now[0] - seen[0], now[1] - seen[1]) == b.stats()
                assert a.launch_info()[2] == b.launch_info()[2] == 6 and a.cull_info() == b.cull_info() and a.cull_info() & 0x57 == 0x57
            finally:
                b.close()
            assert not np.array_equal(bits(got), bits(still))
            s = a.scene_state(["tris", "rest"])
            assert ds.same_bytes(s["tris"][:, :12], posed[:, :12]) and ds.same_bytes(s["rest"], tris[:, :12])
        with pytest.raises(native.NativeError, match=r"moves\[1\] = \[62, 62 \+ 2\) share triangle 62") as e:
            a.pose_parts([(0, 63, SCALE_SHEAR), (62, 2, SCALE_SHEAR)])
        assert e.value.code == native.ERR_INVALID
        assert np.array_equal(bits(render(a, cam, 2, aa=2)), bits(got))
        a.update_triangles(np.ascontiguousarray(tris))
        assert a.scene_state(["rest"])["rest"].size == 0
    finally:
        a.close()


# ---- 6. queries after a pose ------------------------------------------------------------------------------------------------------------------------------------

def test_queries_answer_on_the_posed_scene(native, oracle):
    from rvpt_amd import scene
    (tris, mats, nodes), _ = scene_and_camera("default", 64, 48)
    updates = three_updates(tris)
    posed, current = tris, nodes
    for moves in updates[:2]:
        posed = scene.pose_parts(tris, moves, current=posed)
        current = scene.refit_bvh(current, posed, touched=listed_of(moves))
    records = rq.poisoned(rq.base_rays(posed, 11, counts=(80, 80, 50, 40, 30, 20)))
    want = rq.Statement(oracle, current, posed).answer(records, 0)
    still = rq.Statement(oracle, nodes, tris).answer(records, 0)
    assert not rq.same_bytes(want, still) and 50 < int((want["prim"] != rq.NO_PRIM).sum())
    rng = np.random.RandomState(3)
    org = np.tile(np.array([0.0, 0.0, 0.0], np.float32), (256, 1))
    dirs = rng.normal(size=(256, 3)).astype(np.float32)
    dirs[:, 2] = np.abs(dirs[:, 2]) + 0.5
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True).astype(np.float32)
    seeds = rng.randint(0, 2 ** 31, 256).astype(np.uint32)
    a, b = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH), native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        a.upload_scene(nodes, tris, mats)
        for moves in updates[:2]:
            a.pose_parts(moves)
        got = a.trace_rays_into(records.copy())
        assert rq.same_bytes(got, want), rq.first_difference(got, want)  # prim numbered as before: the stored order
        b.upload_scene(current, posed, mats)
        pa, pb = a.trace_paths(org, dirs, seeds, 6), b.trace_paths(org, dirs, seeds, 6)
        assert pa.tobytes() == pb.tobytes() and int(pa["segments"].sum()) > 256
    finally:
        a.close()
        b.close()


# ---- 7. frames in flight ----------------------------------------------------------------------------------------------------------------------------------------

def test_frames_queued_before_the_update_finish_on_the_old_geometry(native, oracle):
    from rvpt_amd import RenderSettings, scene
    W, H = 64, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    moves = three_updates(tris)[1]
    posed = scene.pose_parts(tris, moves)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, tris, mats)
        for f in range(4):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ctx.pose_parts(moves)  # with four frames queued
        assert ctx.query() is False
        img_old = ctx.read()
        img_new = render(ctx, cam, 2)
    finally:
        ctx.close()
    ref_old, _ = oracle_frames(oracle, (tris, mats, nodes), cam, W, H, "bvh", [0, 1, 2, 3])
    ref_new, _ = oracle_frames(oracle, (posed, mats, scene.refit_bvh(nodes, posed, touched=listed_of(moves))), cam, W, H, "bvh", [0, 1])
    assert np.array_equal(bits(img_old), bits(ref_old[3])) and np.array_equal(bits(img_new), bits(ref_new[1]))


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------------------------

def _raw_pose(native, ctx, rec, k=None, tris=None, mats=None, offset=0):
    """the C call itself: (return code, message); rec: PART_MOVE_DTYPE records or None"""
    keep = None if rec is None else np.ascontiguousarray(rec)
    ptr = None if keep is None else ctypes.c_void_p(keep.ctypes.data + offset)
    t = None if tris is None else np.ascontiguousarray(tris, dtype=np.float32)
    m = None if mats is None else np.ascontiguousarray(mats, dtype=np.float32)
    rc = ctx._L.rvpt_hip_upload_scene(ctx._h, ptr, native.NODES_UPDATE_POSE, None if t is None else t.ctypes.data_as(ctypes.c_void_p), (0 if keep is None else keep.shape[0]) if k is None else k,
                                      None if m is None else m.ctypes.data_as(ctypes.c_void_p), 0 if m is None else m.shape[0])
    return rc, (ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode()


def test_errors_leave_the_scene_and_the_rest_pose_untouched(native):
    import torch
    from rvpt_amd import scene
    W, H = 64, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    n = tris.shape[0]
    eye = np.eye(3, 4)
    ok = scene.part_moves([(0, 5, eye), (10, 5, eye), (20, 5, eye), (30, 5, eye)])
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        rc, msg = _raw_pose(native, ctx, ok)
        assert rc == native.ERR_INVALID and "before any full upload_scene" in msg
        ctx.upload_scene(nodes, tris, mats)
        ctx.pose_parts(three_updates(tris)[0])  # so that there is a rest pose to leave untouched
        img = render(ctx, cam, 2)
        s0 = ctx.scene_state(["tris", "nodes", "rest", "wide"])
        assert s0["rest"].shape == (n, 12)

        def untouched(what):
            s = ctx.scene_state(["tris", "nodes", "rest", "wide"])
            for k in ("tris", "nodes", "rest", "wide"):
                assert ds.same_bytes(s[k], s0[k]), (what, k)
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img)), what

        many = scene.part_moves([(j, 1, eye) for j in range(n)] + [(0, 1, eye)])
        count0, reserved, past, wraps, overlap = ok.copy(), ok.copy(), ok.copy(), ok.copy(), None
        count0["count"][1] = 0
        count0["first"][3] = n  # (position 3 offends too: position 1 is named)
        reserved["reserved"][2, 1] = 7
        past["first"][1], past["count"][1] = n - 2, 3
        past["first"][3] = n + 5
        wraps["first"][2], wraps["count"][2] = 0xFFFFFFFF, 2  # first + count wraps to 1
        overlap = scene.part_moves([(50, 10, eye), (0, 5, eye), (3, 4, eye), (55, 2, eye), (100, 1, eye)])  # (0, 3) and (1, 2) meet: (0, 3) is the smallest pair
        nested = scene.part_moves([(100, 1, eye), (40, 3, eye), (0, 90, eye), (41, 1, eye)])  # (1, 2), (1, 3), (2, 3): (1, 2)
        cases = [((ok, 0), "pose update without parts"),
                 ((many,), f"pose update with {n + 1} parts, the uploaded scene has {n} triangles"),
                 ((None, 4), "pose update without a list"),
                 ((np.concatenate([ok, ok]), 4, None, None, 2), "not 4-byte aligned"),
                 ((ok, None, tris[:4]), "takes no triangles"),
                 ((ok, None, None, mats), "takes no materials"),
                 ((count0,), "moves[1] has a count of 0"),
                 ((reserved,), "moves[2] has the reserved words 0, 7"),
                 ((past,), f"moves[1] = [{n - 2}, {n - 2} + 3) is outside the {n} stored triangles"),
                 ((wraps,), f"moves[2] = [4294967295, 4294967295 + 2) is outside the {n} stored triangles"),
                 ((overlap,), "moves[0] = [50, 50 + 10) and moves[3] = [55, 55 + 2) share triangle 55"),
                 ((nested,), "moves[1] = [40, 40 + 3) and moves[2] = [0, 0 + 90) share triangle 40")]
        for args, what in cases:
            rc, msg = _raw_pose(native, ctx, *args)
            assert rc == native.ERR_INVALID and what in msg, (what, rc, msg)
            untouched(what)
        # the list in device memory
        dev = torch.from_numpy(ok.view(np.uint8).reshape(-1).copy()).to("cuda:0")
        rc = ctx._L.rvpt_hip_upload_scene(ctx._h, ctypes.c_void_p(dev.data_ptr()), native.NODES_UPDATE_POSE, None, ok.shape[0], None, 0)
        assert rc == native.ERR_INVALID and b"device memory" in ctx._L.rvpt_hip_last_error(ctx._h)
        untouched("device list")
        # through the wrapper the library's words arrive as they are
        with pytest.raises(native.NativeError, match=r"moves\[0\] = \[50, 50 \+ 10\) and moves\[3\]") as e:
            ctx.pose_parts(overlap)
        assert e.value.code == native.ERR_INVALID
        rc, msg = _raw_pose(native, ctx, ok)
        assert rc == 0 and msg == ""  # (the same call with a good list is the update, and leaves no message)
    finally:
        ctx.close()


def test_caller_layout_has_no_pose_form(native, monkeypatch):
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    W, H = 64, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(nodes, tris, mats)
        img = render(ctx, cam, 1)
        with pytest.raises(native.NativeError, match="CALLER_LAYOUT") as e:
            ctx.pose_parts([(0, 2, np.eye(3, 4))])
        assert e.value.code == native.ERR_UNSUPPORTED
        assert np.array_equal(bits(render(ctx, cam, 1)), bits(img)) and ctx.scene_state(["rest"])["rest"].size == 0
    finally:
        ctx.close()


# ---- 10. the RVPT mirror ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", ["host", "device-sah"])
def test_renderer_mirror(native, build):
    """RVPT.pose_parts numbers the triangles in the order they were ADDED: the frame equals that of update_triangles(scene.pose_parts(...)) on a second object, the
    mirror's host copies follow, bvh_nodes is the refit of the tree as built, and update_triangles makes what the scene holds the new rest pose."""
    from rvpt_amd import RVPT, scene
    W, H = 64, 48
    tris, mats = scene.default_scene()
    n = tris.shape[0]
    first = [(10, 60, about(centroid(tris, 10, 60), rotation((0, 1, 0), 0.5))), scene.part_move(100, 20, translation=(0.1, 0.2, 0.0))]
    second = [(10, 60, about(centroid(tris, 10, 60), rotation((1, 0, 0), 0.3)))]
    pair = []
    for _ in range(2):
        r = RVPT(W, H, device=0, traversal="bvh", build=build)
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
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
        once = scene.pose_parts(tris, first)
        assert a.pose_parts(first) is None
        b.update_triangles(once)
        got, want = frames()
        assert not np.array_equal(bits(got), bits(still)) and np.array_equal(bits(got), bits(want))
        twice = scene.pose_parts(tris, second, current=once)
        a.pose_parts(second)
        b.update_triangles(twice)
        got, want = frames()
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(np.concatenate(a.triangles), twice) and np.array_equal(a.sorted_triangles, twice[order])
        assert a.bvh_nodes.tobytes() == scene.refit_bvh(built, twice[order]).tobytes() == b.bvh_nodes.tobytes()
        # update_triangles, then a pose: from the triangles just given
        a.update_triangles(once)
        a.pose_parts(second)
        b.update_triangles(scene.pose_parts(once, second))
        got, want = frames()
        assert np.array_equal(bits(got), bits(want))
        with pytest.raises(native.NativeError, match="shares triangle 12"):
            a.pose_parts([(10, 5, np.eye(3, 4)), (12, 1, np.eye(3, 4))])
        with pytest.raises(native.NativeError, match=f"outside the {n}"):
            a.pose_parts([(n - 1, 2, np.eye(3, 4))])
    finally:
        a.shutdown()
        b.shutdown()
