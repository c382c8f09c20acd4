"""K-nearest point queries on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_NEAREST_POINTS_K(k) (Context.closest_points(k=) / closest_points_into(k=)) against
the statement rvpt_amd/scene.py: closest_points_k — a stable sort of the header's per-triangle candidates.  The answer is defined without a walk, so ONE
statement serves every kind of context, every builder, every update form and every tree: whole groups are compared byte for byte, the followers' poisoned in
fields included, no tolerance and no record left out."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _guarded_pose as gp
import _multi_hit as mh
import _nearest as nq
import _nearest_k as nk
import _skin
from _util import identity_camera
from test_gpu_parity import _chain_bvh
from test_ray_query import _mirrored_chain
from test_refit import bits, extent

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = list(range(1, 9))


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    n.load()
    assert n.device_count() >= 1
    return n


def kernel_constant(name, header="rvpt_nearest.h"):
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", (ROOT / "rvpt_amd" / "csrc" / header).read_text()).group(1))


@pytest.fixture(scope="module")
def group_sets(default_scene):
    """k -> (records, the statement's answer in stored order) on the default scene's 143 triangles: the generator's 916 points of every kind, the bound
    variants of 40 of them taken at every j-th answer, thirteen non-finite points: 1 200 to 3 200 groups, no multiple of a run of 64.  Computed once."""
    tris = default_scene[0]
    assert tris.shape[0] == 143
    sets = {k: nk.point_set_k(tris, 7, k) for k in KS}
    for k, (records, want) in sets.items():
        g = want.reshape(-1, k)
        assert 1000 < g.shape[0] < 4000 and g.shape[0] % 64
        filled = (g["prim"] != nq.NO_PRIM).sum(axis=1)
        assert (filled == k).sum() > 900 and (filled == 0).sum() > 50
        if k > 1:
            assert ((filled > 0) & (filled < k)).sum() > 30  # radius queries that end in misses
            assert (g["d2"][:, k - 2] == g["d2"][:, k - 1])[filled == k].sum() > 50  # ties inside the list, at its last slot
    return sets


def ask(native, flags, scene3, records, k, upload=None, lab=None):
    ctx = native.Context(64, 36, 0, 0, 1, flags, lab=lab)
    try:
        if upload is not None:
            upload(ctx)
        else:
            tris, mats, nodes = scene3
            ctx.upload_scene(nodes if flags & 3 else None, tris, mats)
        return ctx.closest_points_into(records.copy(), k=k)
    finally:
        ctx.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BVH_ORDERED", "TRAVERSAL_BVH|BVH_PER_LANE", "TRAVERSAL_BRUTE"])
def test_every_k_on_every_context(native, default_scene, group_sets, flags, k):
    """Every kind of context gives the statement's bytes at every k — the tree walk and the brute-force kernel alike — for a few thousand groups, for 45 groups
    (fewer than a wave) and for one group."""
    records, want = group_sets[k]
    fl = 0
    for name in flags.split("|"):
        fl |= getattr(native, name)
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
        got = ctx.closest_points_into(records.copy(), k=k)
        nk.check_k(got, want, records, k, f"{flags}, k = {k}")
        assert (got.reshape(-1, k)["prim"][-12:] == nq.NO_PRIM).all()  # the non-finite dozen
        few, few_want = records[-45 * k:], want[-45 * k:]
        nk.check_k(ctx.closest_points_into(few.copy(), k=k), few_want, few, k, f"{flags}, k = {k}, 45 groups")
        one = int(np.flatnonzero(want.reshape(-1, k)["prim"][:, 0] != nq.NO_PRIM)[0])
        sub = records[one * k:(one + 1) * k]
        nk.check_k(ctx.closest_points_into(sub.copy(), k=k), want[one * k:(one + 1) * k], sub, k, f"{flags}, k = {k}, one group")
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_k_1_is_format_4(native, default_scene, group_sets, flags):
    """FORMAT_NEAREST_POINTS_K(1) returns format 4's bytes on the same records, and speaks with format 4's messages"""
    records, want = group_sets[1]
    tris, mats, nodes = default_scene
    fl = getattr(native, flags)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
        plain = ctx.closest_points_into(records.copy())
        as_k = ctx.closest_points_into(records.copy(), k=1)
        assert plain.tobytes() == as_k.tobytes() == want.tobytes()
        buf = records[:2].copy()
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_NEAREST_POINTS_K(1), buf.ctypes.data_as(ctypes.c_void_p), 49)
        said = ctx._L.rvpt_hip_last_error(ctx._h)
        assert rc == native.ERR_INVALID and b"point query: dst_bytes 49 is not a multiple of the 48 bytes of a rvpt_point_hit" in said and b"k =" not in said
        assert buf.tobytes() == records[:2].tobytes()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def cornell_sets():
    from rvpt_amd import scene
    tris, mats = scene.cornell_scene(2)
    assert tris.shape[0] == 2300
    tris = np.ascontiguousarray(tris[np.random.RandomState(2).permutation(tris.shape[0])])
    sets = {k: nk.point_set_k(tris, 17, k, counts=(200, 60, 60, 60, 30), variants_of=20) for k in (3, 8)}
    for k, (_, want) in sets.items():
        g = want.reshape(-1, k)
        assert ((g["prim"][:, k - 1] != nq.NO_PRIM) & (g["d2"][:, k - 2] == g["d2"][:, k - 1])).sum() > 20  # ties the caller's numbers must break
    return tris, mats, sets


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_three_builders_give_the_same_bytes(native, cornell_sets, method, k):
    """build_scene on 2 300 shuffled triangles: prim numbers the CALLER'S order and ties are broken on it, so the three builders return the same bytes — the
    statement's on the caller's array."""
    tris, mats, sets = cornell_sets
    records, want = sets[k]
    got = ask(native, native.TRAVERSAL_BVH, None, records, k, upload=lambda ctx: ctx.build_scene(tris, mats, method) == method or pytest.fail("fell back"))
    nk.check_k(got, want, records, k, f"{method}, k = {k}")


@pytest.mark.parametrize("k", [2, 3, 5])
@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_stacked_duplicates_are_cut_by_k_in_number_order(native, flags, k):
    """The multi-hit tests' 12 layers with four exact duplicates: a point on the quads' shared diagonal in front of a doubled layer has FOUR candidates at one
    d2.  k = 2 and 3 cut them, k = 5 holds them all and one more; the order inside the tie is the order of the numbers."""
    from rvpt_amd import scene
    tris, zs = mh.layered_scene()
    mats = scene.default_materials()
    points = np.concatenate([nk.diagonal_points(zs), nq.base_points(tris, 23, counts=(60, 20, 20, 20, 8))])
    n_diag = nk.diagonal_points(zs).shape[0]
    assert n_diag == 5 * len(set(zs[[j for j in range(len(zs)) if (zs == zs[j]).sum() == 4]].tolist())) == 10
    records = nk.groups(points, k)
    want = nk.answer_k(tris, records, k)
    five = scene.closest_points_k(tris, points["point"][:n_diag], 5)
    assert (five["d2"][:, 0] == five["d2"][:, 3]).all() and (five["d2"][:, 3] < five["d2"][:, 4]).all()  # four at one distance, then the next
    assert (np.diff(five["prim"][:, :4].astype(np.int64), axis=1) > 0).all()
    g = want.reshape(-1, k)[:n_diag]
    assert (g["prim"][:, :min(k, 4)] == five["prim"][:, :min(k, 4)]).all()
    fl = getattr(native, flags)
    if fl & 3:
        got = ask(native, fl, None, records, k, upload=lambda ctx: ctx.build_scene(tris, mats, "sah"))
    else:
        got = ask(native, fl, (tris, mats, None), records, k)
    nk.check_k(got, want, records, k, f"layers, {flags}, k = {k}")


@pytest.mark.parametrize("k", [4, 8])
def test_a_callers_tree_with_loose_boxes(native, default_scene, group_sets, k):
    """Boxes grown at random still contain their vertices: the walk visits more and answers the same."""
    records, want = group_sets[k]
    tris, mats, nodes = default_scene
    loose = nq.grown_boxes(nodes, 5)
    assert loose.tobytes() != np.ascontiguousarray(nodes).tobytes()
    nk.check_k(ask(native, native.TRAVERSAL_BVH, (tris, mats, loose), records, k), want, records, k, f"loose boxes, k = {k}")


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("shape", ["chain", "mirrored"])
def test_the_overflow_stack(native, shape, k):
    """The chain of 48 leaves of the point queries' case 4: the tree's height sizes the stack at 48 slots, of which kQueryLdsLevels = 8 live in LDS; from beyond
    the far end every leaf on the way is stacked while the list is not yet full.  Both leanings, points at both ends."""
    from rvpt_amd import scene
    assert kernel_constant("kQueryLdsLevels", "rvpt_query.h") == 8
    rng = np.random.RandomState(11)
    quads = []
    for i in range(24):
        z, s, c = 1.0 + 0.25 * i, 0.3 + 0.05 * i, rng.uniform(-0.5, 0.5, 2)
        p = [(c[0] - s, c[1] - s, z), (c[0] + s, c[1] - s, z), (c[0] + s, c[1] + s, z), (c[0] - s, c[1] + s, z)]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    tris = scene.make_triangles(quads, 0)
    mats = scene.default_materials()
    nodes = _chain_bvh(tris) if shape == "chain" else _mirrored_chain(tris)
    base = nq.base_points(tris, 3, counts=(120, 30, 30, 30, 10))
    ends = nq.make_records([(x, y, z) for z in (-3.0, 0.5, 7.5, 12.0) for x in (-0.4, 0.0, 0.7) for y in (-0.2, 0.5)])
    with np.errstate(all="ignore"):
        points = np.concatenate([base, nk.with_bound_variants_at(base[:20], tris, k)[20:], ends])
    records = nk.groups(points, k)
    want = nk.answer_k(tris, records, k)
    g = want.reshape(-1, k)
    assert (g["prim"][-6:, 0] >= 46).all() and (g["prim"][-24:-18, 0] <= 1).all()  # the ends of the chain answer the ends of the line
    nk.check_k(ask(native, native.TRAVERSAL_BVH, (tris, mats, nodes), records, k), want, records, k, f"{shape}, k = {k}")


def test_brute_force_tiles_wrap(native):
    """kNearestTileTris = 512 triangle rows per LDS tile: 2 * 512 + 37 triangles are two tiles and a tail; every tile answers somebody, and some group's eight
    entries come from two tiles."""
    from rvpt_amd import scene
    tile = kernel_constant("kNearestTileTris")
    assert tile == 512
    tris, mats = scene.heightfield_scene(cells=24)  # 1152 triangles
    tris = np.ascontiguousarray(tris[:2 * tile + 37])
    records, want = nk.point_set_k(tris, 13, 8, counts=(150, 50, 50, 50, 20), variants_of=20)
    g = want.reshape(-1, 8)
    full = g["prim"][:, 7] != nq.NO_PRIM
    tiles = g["prim"][full] // tile
    assert (tiles == 0).any() and (tiles == 1).any() and (tiles == 2).any() and (tiles.min(axis=1) != tiles.max(axis=1)).sum() > 10
    nk.check_k(ask(native, native.TRAVERSAL_BRUTE, (tris, mats, None), records, 8), want, records, 8, "brute force, three tiles")


@pytest.mark.parametrize("form", ["plain", "sparse", "pose", "skin", "guarded pose"])
@pytest.mark.parametrize("traversal", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_queries_answer_for_the_mesh_as_the_last_update_left_it(native, traversal, form):
    """After update_triangles (plain, indices=), pose_parts, bind_skin + skin, and a guarded pose update that rebuilds, as in the point queries' case 6: the
    statement on the triangles the update form's own numpy statement gives, in the caller's order — which is also the numbering after the rebuild.  k = 4."""
    from rvpt_amd import scene
    k = 4
    tris, mats = scene.default_scene()
    n = tris.shape[0]
    fl = getattr(native, traversal)
    records = nk.groups(nq.base_points(tris, 19, counts=(400, 80, 80, 80, 30)), k)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        assert ctx.build_scene(tris, mats, "lbvh") == "lbvh"
        before = ctx.closest_points_into(records.copy(), k=k)
        nk.check_k(before, nk.answer_k(tris, records, k), records, k, f"{form}: before")
        if form == "plain":
            moved = scene.wobble(tris, 1.9, 0.1 * extent(tris))
            ctx.update_triangles(moved)
        elif form == "sparse":
            idx = np.random.RandomState(7).permutation(n)[:n // 3]
            moved = tris.copy()
            moved[idx, :12] = scene.wobble(tris, 1.9, 0.1 * extent(tris))[idx, :12]
            ctx.update_triangles(moved[idx], indices=idx)
        elif form == "pose":
            f, c = gp.part_of(n)
            moves = [gp.turned(tris, f, c, 25.0), gp.carried(tris, *gp.second_part_of(n))]
            moved = scene.pose_parts(tris, moves)
            ctx.pose_parts(moves)
        elif form == "skin":
            rec, m = _skin.weights(tris, 6), _skin.bones(tris, 6, 0.4)
            moved = scene.skin_triangles(tris, rec, m)
            ctx.bind_skin(rec)
            ctx.skin(m)
        else:
            f, c = gp.part_of(n)
            moves = [gp.turned(tris, f, c, 90.0)]
            step = gp.step(gp.built(tris, "lbvh"), moves, 1.02, "lbvh")
            assert step.rebuilt
            moved = step.state.current
            report = ctx.pose_parts(moves, rebuild_above=1.02)
            assert report is None if traversal == "TRAVERSAL_BRUTE" else report.rebuilt
        got = ctx.closest_points_into(records.copy(), k=k)
    finally:
        ctx.close()
    nk.check_k(got, nk.answer_k(moved, records, k), records, k, form)
    assert not nq.same_bytes(got, before)


@pytest.mark.parametrize("idx", [13, 43])
def test_hostile_scenes_for_equality_only(native, idx):
    """Cases 13 and 43 of the hostile fuzz's slice (tools/fuzz_bvh.py): duplicates and zero-area triangles, and a scale of 2^20.  Nothing is asserted of the
    geometry: the device-built tree, a brute-force context and the statement give the same bytes at k = 5."""
    sys.path.insert(0, str(ROOT / "tools"))
    import fuzz_bvh
    k = 5
    case = fuzz_bvh.reduced_case(606, idx, 64, 36, max_tris=256)
    tris, mats = np.ascontiguousarray(case["tris"], dtype=np.float32), case["mats"]
    assert (case["kind"], case["k"]) == {13: ("soup_dup", -3), 43: ("soup", 20)}[idx]
    with np.errstate(all="ignore"):
        records, want = nk.point_set_k(tris, idx, k, counts=(150, 40, 40, 40, 15), variants_of=20)
    method = fuzz_bvh.METHODS[idx % 3]
    got = ask(native, native.TRAVERSAL_BVH, None, records, k, upload=lambda ctx: ctx.build_scene(tris, mats, method))
    nk.check_k(got, want, records, k, f"case {idx}, {method}")
    nk.check_k(ask(native, native.TRAVERSAL_BRUTE, (tris, mats, None), records, k), want, records, k, f"case {idx}, brute force")


def test_device_records_the_errors_and_the_empty_scene(native, default_scene, group_sets):
    """A torch tensor on cuda:0, in place, and a (n, k) host array: the bytes a flat host query returns.  48 * k * n + 48 bytes (the message gives k), a view 4
    bytes in, no scene, formats 48 and 57: INVALID, memory untouched.  The empty scene: k miss slots for every group.  closest_points(k=) builds its groups."""
    import torch
    k = 3
    records, want = group_sets[k]
    tris, mats, nodes = default_scene
    n = records.shape[0] // k
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        host12 = torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12))
        with pytest.raises(native.NativeError, match="point query before any full upload_scene.*no scene to ask") as e:
            ctx.closest_points_into(host12.clone(), k=k)
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        dev = host12.to("cuda:0")
        assert ctx.closest_points_into(dev, k=k) is dev
        nk.check_k(dev.cpu().numpy().view(native.POINT_HIT_DTYPE).reshape(-1), want, records, k, "device records")
        two_d = records.copy().reshape(n, k)  # a (n, k) host array
        assert ctx.closest_points_into(two_d, k=k) is two_d
        nk.check_k(two_d, want, records, k, "a (n, k) array")
        flat = host12.to("cuda:0").reshape(-1)  # a view that starts 4 bytes in: device records need 16-byte alignment
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="point records on the device need 16-byte alignment") as e:
            ctx.closest_points_into(flat[1:1 + 12 * 2 * k].reshape(2 * k, 12), k=k)
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        buf = records[:5 * k + 1].copy()  # 48 * k * 5 + 48 bytes, through the C call
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_NEAREST_POINTS_K(k), buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes)
        said = ctx._L.rvpt_hip_last_error(ctx._h)
        assert rc == native.ERR_INVALID and b"point query with k = 3" in said and str(buf.nbytes).encode() in said and b"multiple" in said and b"rvpt_point_hit" in said
        assert buf.tobytes() == records[:5 * k + 1].tobytes()
        for fmt in (48, 57):
            rc = ctx._L.rvpt_hip_read(ctx._h, fmt, buf.ctypes.data_as(ctypes.c_void_p), 48 * k * 5)
            assert rc != 0 and f"unknown format {fmt}".encode() in ctx._L.rvpt_hip_last_error(ctx._h) and buf.tobytes() == records[:5 * k + 1].tobytes()
        ctx.closest_points_into(records[:k].copy(), k=k)  # a successful query leaves last_error as it was
        assert b"unknown format 57" in ctx._L.rvpt_hip_last_error(ctx._h)
        assert ctx.closest_points_into(records[:0].copy(), k=k).shape == (0,)
        assert ctx.closest_points_into(torch.zeros((0, 12), device="cuda:0"), k=k).shape == (0, 12)
        # closest_points builds the groups itself: the point repeated in every record, the distance squared
        g = want.reshape(n, k)
        some = np.flatnonzero(np.isinf(g["max_d2"][:, 0]) & np.isfinite(g["point"][:, 0]).all(axis=1))[:50]
        out = ctx.closest_points(g["point"][some, 0], k=k)
        assert out.shape == (50, k) and out.dtype == native.POINT_HIT_DTYPE
        for name in nq.OUT_FIELDS:
            assert out[name].tobytes() == np.ascontiguousarray(g[name][some]).tobytes(), name
        assert (out["point"] == g["point"][some, :1]).all() and np.isinf(out["max_d2"]).all()
        # the empty scene answers every group with k misses
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        empty = ctx.closest_points_into(records.copy(), k=k)
        assert (empty["prim"] == nq.NO_PRIM).all()
        nk.check_k(empty, nk.answer_k(np.zeros((0, 16), np.float32), records, k), records, k, "the empty scene")
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_a_query_leaves_frames_untouched(native, default_scene, group_sets, flags):
    """Two accumulated frames, a k-nearest query, a third frame: image, stats, the timing's dispatch count, launch_info, cull_info and last_error equal a
    context that never asked."""
    from rvpt_amd import RenderSettings
    k = 8
    records, _ = group_sets[k]
    tris, mats, nodes = default_scene
    fl = getattr(native, flags) | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for asks in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
            if asks:
                ctx.closest_points_into(records[:300 * k].copy(), k=k)  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.closest_points_into(records[:1000 * k].copy(), k=k)  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info(), ctx._L.rvpt_hip_last_error(ctx._h)))
        finally:
            ctx.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("traversal", ["bvh", "brute"])
def test_rvpt_closest_points_k_numbers_the_triangles_as_they_were_added(native, traversal):
    """RVPT.closest_points(k=) over a host-built tree: the host builder reorders the triangles, the mirror maps prim of every filled slot back.  A point lifted
    off a triangle's centroid finds that triangle first, by the number it was added under; the k entries are the statement's on the added order wherever their
    distances are distinct (over a host-built tree ties are broken on the stored number, before the renumbering)."""
    from rvpt_amd import RVPT, scene
    k = 4
    tris, mats = scene.heightfield_scene(cells=12)  # 288 triangles, none folded onto another
    r = RVPT(64, 36, device=0, traversal=traversal)
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        v = tris.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
        nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        lift = 1e-3 * extent(tris)
        pts = (v.mean(axis=1) + lift * nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
        rec = r.closest_points(pts, k=k)
        assert rec.shape == (tris.shape[0], k) and rec.dtype == native.POINT_HIT_DTYPE
        assert rec["prim"][:, 0].tolist() == list(range(tris.shape[0])) and (rec["region"][:, 0] == 0).all()
        want = scene.closest_points_k(tris, pts, k + 1)
        distinct = (np.diff(want["d2"], axis=1) > 0).all(axis=1)  # no tie among the first k + 1: the order of the numbers plays no part
        assert distinct.sum() > 100
        for name in nq.OUT_FIELDS:
            assert np.ascontiguousarray(rec[name][distinct]).tobytes() == np.ascontiguousarray(want[name][distinct][:, :k]).tobytes(), name
        assert (np.sort(rec["d2"], axis=1) == rec["d2"]).all() and (rec["d2"] == want["d2"][:, :k]).all()  # the distances are the statement's everywhere
        near = r.closest_points(pts, max_dist=0.5 * lift, k=k)
        assert (near["prim"] == native.NO_PRIM).all() and near.shape == (tris.shape[0], k)
    finally:
        r.shutdown()
