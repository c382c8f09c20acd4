"""Point queries on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_NEAREST_POINTS (Context.closest_points / closest_points_into) against the statement
rvpt_amd/scene.py: closest_points — brute force over the header's per-triangle arithmetic.  The answer is defined without a walk, so ONE statement serves every
kind of context, every builder, every update form and every tree: whole records are compared byte for byte, no tolerance and no record left out."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

import _guarded_pose as gp
import _nearest as nq
import _skin
from _util import identity_camera
from test_gpu_parity import _chain_bvh
from test_ray_query import _mirrored_chain
from test_refit import bits, extent

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


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
def point_set(default_scene):
    """(records, the statement's answer in stored order) on the default scene's 143 triangles: the generator's points of every kind with the seven bound
    variants of every answered one and a dozen non-finite points, filled up with uniform points to 64 k + 1 records.  Computed once, never changed."""
    tris = default_scene[0]
    assert tris.shape[0] == 143
    records, _ = nq.point_set(tris, 7)
    fill = 65537 - records.shape[0]
    assert fill > 0
    more = nq.base_points(tris, 8, counts=(fill - 16, 0, 0, 0, 0))
    records = nq.poisoned(np.concatenate([more, records]))  # (the non-finite dozen stays last)
    assert records.shape[0] == 65537
    want = nq.answer(tris, records)
    records.setflags(write=False)
    want.setflags(write=False)
    hit = want["prim"] != nq.NO_PRIM
    assert hit.sum() > 60000 and (~hit).sum() > 1000 and set(np.unique(want["region"][hit]).tolist()) == set(range(7))
    return records, want


def ask(native, flags, scene3, records, upload=None, lab=None):
    ctx = native.Context(64, 36, 0, 0, 1, flags, lab=lab)
    try:
        if upload is not None:
            upload(ctx)
        else:
            tris, mats, nodes = scene3
            ctx.upload_scene(nodes if flags & 3 else None, tris, mats)
        return ctx.closest_points_into(records.copy())
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BVH_ORDERED", "TRAVERSAL_BVH|BVH_PER_LANE", "TRAVERSAL_BRUTE"])
def test_queries_answer_as_the_statement(native, default_scene, point_set, flags):
    """Case 1.  Every kind of context gives the statement's bytes — the tree walk and the brute-force kernel alike — for 64 k + 1 records (more than the
    persistent grid holds at once, and no multiple of a run of 64) and for fewer records than a wave."""
    records, want = point_set
    fl = 0
    for name in flags.split("|"):
        fl |= getattr(native, name)
    got = ask(native, fl, default_scene, records)
    nq.check(got, want, records, flags)
    assert (got["prim"][-12:] == nq.NO_PRIM).all()
    few = records[-45:]
    nq.check(ask(native, fl, default_scene, few), want[-45:], few, flags + ", 45 records")


@pytest.fixture(scope="module")
def cornell_set():
    from rvpt_amd import scene
    tris, mats = scene.cornell_scene(2)
    assert tris.shape[0] == 2300
    tris = np.ascontiguousarray(tris[np.random.RandomState(2).permutation(tris.shape[0])])
    records, want = nq.point_set(tris, 17, counts=(200, 60, 60, 60, 30))
    assert (want["prim"] != nq.NO_PRIM).sum() > 1000
    return tris, mats, records, want


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_prim_is_the_callers_index_whichever_builder_made_the_tree(native, cornell_set, method):
    """Case 2.  build_scene on 2 300 shuffled triangles: prim numbers the CALLER'S order and ties are broken on it, so the three builders return the same bytes —
    the statement's on the caller's array."""
    tris, mats, records, want = cornell_set
    got = ask(native, native.TRAVERSAL_BVH, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, method) == method or pytest.fail("fell back"))
    nq.check(got, want, records, method)


def test_a_callers_tree_with_loose_boxes(native, default_scene, point_set):
    """Case 3.  Boxes grown at random still contain their vertices: the walk visits more and answers the same."""
    records, want = point_set
    tris, mats, nodes = default_scene
    loose = nq.grown_boxes(nodes, 5)
    assert loose.tobytes() != np.ascontiguousarray(nodes).tobytes()
    sub = records[-6000:]
    nq.check(ask(native, native.TRAVERSAL_BVH, (tris, mats, loose), sub), want[-6000:], sub, "loose boxes")


@pytest.mark.parametrize("shape", ["chain", "mirrored"])
def test_the_overflow_stack(native, shape):
    """Case 4.  A chain of 48 leaves: the tree's height sizes the stack at 48 slots, of which kQueryLdsLevels = 8 live in LDS.  The walk descends into the nearer
    child and stacks the farther: for a point beyond the far end of the chain the REST of the chain is the nearer child at every level, every leaf on the way is
    stacked (best is still +inf), and the 40 global levels are used; from the near end the stack stays shallow.  Both leanings, points at both ends."""
    from rvpt_amd import scene
    assert kernel_constant("kQueryLdsLevels", "rvpt_query.h") == 8
    rng = np.random.RandomState(11)
    quads = []
    for k in range(24):
        z, s, c = 1.0 + 0.25 * k, 0.3 + 0.05 * k, rng.uniform(-0.5, 0.5, 2)
        p = [(c[0] - s, c[1] - s, z), (c[0] + s, c[1] - s, z), (c[0] + s, c[1] + s, z), (c[0] - s, c[1] + s, z)]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    tris = scene.make_triangles(quads, 0)
    mats = scene.default_materials()
    nodes = _chain_bvh(tris) if shape == "chain" else _mirrored_chain(tris)
    base = nq.base_points(tris, 3, counts=(120, 30, 30, 30, 10))
    ends = nq.make_records([(x, y, z) for z in (-3.0, 0.5, 7.5, 12.0) for x in (-0.4, 0.0, 0.7) for y in (-0.2, 0.5)])
    records = np.concatenate([base, ends])
    want = nq.answer(tris, records)
    assert (want["prim"][-6:] >= 46).all() and (want["prim"][-24:-18] <= 1).all()  # the ends of the chain answer the ends of the line
    nq.check(ask(native, native.TRAVERSAL_BVH, (tris, mats, nodes), records), want, records, shape)


def test_brute_force_tiles_wrap(native):
    """Case 5.  kNearestTileTris = 512 triangle rows per LDS tile: 2 * 512 + 37 triangles are two tiles and a tail, and every tile answers somebody."""
    from rvpt_amd import scene
    tile = kernel_constant("kNearestTileTris")
    assert tile == 512
    tris, mats = scene.heightfield_scene(cells=24)  # 1152 triangles
    tris = np.ascontiguousarray(tris[:2 * tile + 37])
    records, want = nq.point_set(tris, 13, counts=(150, 50, 50, 50, 20))
    hit = want["prim"][want["prim"] != nq.NO_PRIM]
    assert (hit < tile).any() and ((hit >= tile) & (hit < 2 * tile)).any() and (hit >= 2 * tile).any()
    nq.check(ask(native, native.TRAVERSAL_BRUTE, (tris, mats, None), records), want, records, "brute force, three tiles")


@pytest.mark.parametrize("form", ["plain", "sparse", "pose", "skin", "guarded pose"])
@pytest.mark.parametrize("traversal", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_queries_answer_for_the_mesh_as_the_last_update_left_it(native, traversal, form):
    """Case 6.  After update_triangles (plain, indices=), pose_parts, bind_skin + skin, and a guarded pose update that rebuilds: the statement on the triangles
    the update form's own numpy statement gives (scene.pose_parts, scene.skin_triangles), in the caller's order — which is also the numbering after the rebuild."""
    from rvpt_amd import scene
    tris, mats = scene.default_scene()
    n = tris.shape[0]
    fl = getattr(native, traversal)
    records = nq.base_points(tris, 19, counts=(400, 80, 80, 80, 30))
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        assert ctx.build_scene(tris, mats, "lbvh") == "lbvh"
        before = ctx.closest_points_into(records.copy())
        nq.check(before, nq.answer(tris, records), records, f"{form}: before")
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
            moves = [gp.turned(tris, f, c, 90.0)]  # a tenth of the mesh turned a quarter: the posed tree costs 1.050 of the built one
            step = gp.step(gp.built(tris, "lbvh"), moves, 1.02, "lbvh")
            assert step.rebuilt
            moved = step.state.current
            report = ctx.pose_parts(moves, rebuild_above=1.02)
            assert report is None if traversal == "TRAVERSAL_BRUTE" else report.rebuilt
        got = ctx.closest_points_into(records.copy())
    finally:
        ctx.close()
    nq.check(got, nq.answer(moved, records), records, form)
    assert not nq.same_bytes(got, before)


@pytest.mark.parametrize("idx", [13, 38, 43, 22])
def test_hostile_scenes_for_equality_only(native, idx):
    """Case 7.  The hostile fuzz's scenes (tools/fuzz_bvh.py, the slice of tests/test_fuzz_bvh.py): duplicates and zero-area triangles (13, 38: soup_dup, the
    latter scaled by 2^18), scales of 2^20 (43) and 2^-20 (22).  Nothing is asserted of the geometry: the device-built tree, a brute-force context and the
    statement give the same bytes."""
    sys.path.insert(0, str(ROOT / "tools"))
    import fuzz_bvh
    case = fuzz_bvh.reduced_case(606, idx, 64, 36, max_tris=256)
    tris, mats = np.ascontiguousarray(case["tris"], dtype=np.float32), case["mats"]
    assert (case["kind"], case["k"]) == {13: ("soup_dup", -3), 38: ("soup_dup", 18), 43: ("soup", 20), 22: ("model", -20)}[idx]
    with np.errstate(all="ignore"):
        records, want = nq.point_set(tris, idx, counts=(150, 40, 40, 40, 15))
    method = fuzz_bvh.METHODS[idx % 3]
    got = ask(native, native.TRAVERSAL_BVH, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, method))
    nq.check(got, want, records, f"case {idx}, {method}")
    nq.check(ask(native, native.TRAVERSAL_BRUTE, (tris, mats, None), records), want, records, f"case {idx}, brute force")


def test_device_records_and_the_errors(native, default_scene, point_set):
    """Case 8.  A torch tensor on cuda:0, in place: the bytes a host query returns.  A view 4 bytes in, 47 and 49 bytes, no scene: INVALID, memory untouched.
    n = 0 and n = 1.  The empty scene: all misses, every out field written.  closest_points squares its max_dist."""
    import torch
    records, want = point_set
    records, want = records[-8000:], want[-8000:]
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        host12 = torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12))
        with pytest.raises(native.NativeError, match="point query before any full upload_scene.*no scene to ask") as e:
            ctx.closest_points_into(host12.clone())
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        dev = host12.to("cuda:0")
        assert ctx.closest_points_into(dev) is dev
        nq.check(dev.cpu().numpy().view(native.POINT_HIT_DTYPE).reshape(-1), want, records, "device records")
        host_t = host12.clone()  # a host tensor goes the host way
        ctx.closest_points_into(host_t)
        nq.check(host_t.numpy().view(native.POINT_HIT_DTYPE).reshape(-1), want, records, "host tensor")
        flat = host12.to("cuda:0").reshape(-1)  # a view that starts 4 bytes in: device records need 16-byte alignment
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="point records on the device need 16-byte alignment") as e:
            ctx.closest_points_into(flat[1:1 + 12 * 5].reshape(5, 12))
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        buf = records[:2].copy()
        for nbytes in (47, 49):  # byte counts that are no whole number of records, through the C call
            rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_NEAREST_POINTS, buf.ctypes.data_as(ctypes.c_void_p), nbytes)
            said = ctx._L.rvpt_hip_last_error(ctx._h)
            assert rc == native.ERR_INVALID and b"point query" in said and b"multiple" in said and b"rvpt_point_hit" in said
            assert buf.tobytes() == records[:2].tobytes()
        ctx.closest_points_into(records[:1].copy())  # a successful query leaves last_error as it was
        assert b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h)
        assert ctx.closest_points_into(records[:0].copy()).shape == (0,)
        assert ctx.closest_points_into(torch.zeros((0, 12), device="cuda:0")).shape == (0, 12)
        k = int(np.flatnonzero(want["prim"] != nq.NO_PRIM)[0])
        nq.check(ctx.closest_points_into(records[k:k + 1].copy()), want[k:k + 1], records[k:k + 1], "one record")
        one = torch.from_numpy(records[k:k + 1].copy().view(np.float32).reshape(1, 12)).to("cuda:0")
        nq.check(ctx.closest_points_into(one).cpu().numpy().view(native.POINT_HIT_DTYPE).reshape(-1), want[k:k + 1], records[k:k + 1], "one device record")
        # closest_points builds the records itself: the distance goes in squared, and a bound just below the distance finds nothing
        r = want[k]
        dist = float(np.sqrt(np.float64(r["d2"])))
        out = ctx.closest_points(r["point"], 2 * dist + 1)
        assert out.dtype == native.POINT_HIT_DTYPE and out[0]["prim"] == r["prim"] and bits(out["d2"])[0] == bits(want["d2"])[k]
        assert bits(out["closest"][0]).tolist() == bits(r["closest"]).tolist()
        if dist > 0:
            assert ctx.closest_points(r["point"], 0.5 * dist)[0]["prim"] == nq.NO_PRIM
        # the empty scene answers every record with a miss
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        empty = ctx.closest_points_into(records.copy())
        assert (empty["prim"] == nq.NO_PRIM).all()
        nq.check(empty, nq.answer(np.zeros((0, 16), np.float32), records), records, "the empty scene")
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_a_query_leaves_frames_untouched(native, default_scene, point_set, flags):
    """Case 9.  Two accumulated frames, a query, a third frame: image, stats, the timing's dispatch count, launch_info, cull_info and last_error equal a
    context that never asked."""
    from rvpt_amd import RenderSettings
    records, _ = point_set
    tris, mats, nodes = default_scene
    fl = getattr(native, flags) | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for asks in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
            if asks:
                ctx.closest_points_into(records[:300].copy())  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.closest_points_into(records[:5000].copy())  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info(), ctx._L.rvpt_hip_last_error(ctx._h)))
        finally:
            ctx.close()
    assert out[0] == out[1]


def test_any_rank_of_a_partition_answers(native, default_scene, point_set):
    """Case 10.  tile_world = 2 without a communicator: rank 1's context holds the whole scene and returns case 1's bytes."""
    records, want = point_set
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 1, 2, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, tris, mats)
        nq.check(ctx.closest_points_into(records[-3000:].copy()), want[-3000:], records[-3000:], "rank 1 of 2")
    finally:
        ctx.close()


@pytest.mark.parametrize("traversal", ["bvh", "brute"])
def test_rvpt_closest_points_numbers_the_triangles_as_they_were_added(native, traversal):
    """Case 11.  RVPT.closest_points: a point lifted off each triangle's centroid along its normal finds that triangle, by the number it was added under (the
    host builder reorders the triangles; the mirror maps prim back), at the lifted distance."""
    from rvpt_amd import RVPT, scene
    tris, mats = scene.heightfield_scene(cells=12)  # 288 triangles, none folded onto another
    r = RVPT(64, 36, device=0, traversal=traversal)
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        v = tris.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
        nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        area2 = np.linalg.norm(nrm, axis=1)
        lift = 1e-3 * extent(tris)
        pts = v.mean(axis=1) + lift * nrm / area2[:, None]
        rec = r.closest_points(pts)
        assert rec.dtype == native.POINT_HIT_DTYPE and (rec["region"] == 0).all()
        assert rec["prim"].tolist() == list(range(tris.shape[0]))
        assert np.allclose(np.sqrt(rec["d2"].astype(np.float64)), lift, rtol=1e-3)
        assert (r.closest_points(pts, max_dist=0.5 * lift)["prim"] == native.NO_PRIM).all()
    finally:
        r.shutdown()
