"""The geometry read-back on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_TRIANGLES (Context.read_triangles / read_triangles_into) against the rows
tests/_scene_model.py states (Model.current, in update order), and with RVPT_HIP_FORMAT_SURFACE_POINTS (Context.surface_points / surface_points_into) against
the statement rvpt_amd/scene.py: surface_points.  Whole rows and whole records are compared byte for byte: no tolerance anywhere."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

import _guarded_pose as gp
import _nearest as nq
import _ray_query as rq
import _scene_model as sm
import _skin
from _util import identity_camera

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import fuzz_updates as fu  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ["TRAVERSAL_BVH", "TRAVERSAL_BVH_ORDERED", "TRAVERSAL_BVH|BVH_PER_LANE", "TRAVERSAL_BRUTE"]  # the four context kinds of tests/test_nearest.py
NO_PRIM = 0xFFFFFFFF
POISON = 0xCD


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    n.load_lab()
    assert n.device_count() >= 1
    return n


def flags_of(native, kind):
    fl = 0
    for name in kind.split("|"):
        fl |= getattr(native, name)
    return fl


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def first_row(got, want):
    g, w = np.ascontiguousarray(got).view(np.uint32).reshape(got.shape[0], -1), np.ascontiguousarray(want).view(np.uint32).reshape(want.shape[0], -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    return "no difference" if bad.size == 0 else f"{bad.size} of {g.shape[0]} differ, the first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def marked(tris, seed):
    """the rows with NaN payloads of their own in the three w lanes (quiet, signalling and negative ones) and a mat_id row of their own"""
    t = np.array(tris, dtype=np.float32).reshape(-1, 16)
    n = t.shape[0]
    w = t.view(np.uint32)
    k = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)
    w[:, 3] = np.uint32(0x7FC00000) | (k & np.uint32(0x3FFFFF))
    w[:, 7] = np.uint32(0x7F800001) + (k >> np.uint32(12))          # signalling payloads
    w[:, 11] = np.uint32(0xFFC00000) | ((k >> np.uint32(5)) & np.uint32(0x3FFFFF))
    t[:, 12] = np.arange(n) % 2
    t[:, 13], t[:, 14] = np.arange(n) + 0.5, -np.arange(n) - 0.25
    w[:, 15] = np.uint32(0x7FC00000) | (k >> np.uint32(10))
    assert np.isnan(t[:, [3, 7, 11, 15]]).all()
    return t


def torch_rows(n, device="cuda:0"):
    import torch
    return torch.full((n, 16), float("nan"), dtype=torch.float32, device=device)


# ---- format 5 ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_an_ordinary_upload_reads_back_byte_for_byte(native, kind):
    """Case 1.  The uploaded array, w lanes (NaN payloads) and mat_id rows included, into a host array and a device tensor; 64 triangles are 256 quads, one
    work-group of the quad-per-thread scatter, hence 63, 64, 65 (a context without a permutation copies, and must agree), 1 and 257."""
    import torch
    from rvpt_amd import scene
    import _device_state as ds
    fl = flags_of(native, kind)
    mats = scene.default_materials()
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        for n in (1, 63, 64, 65, 257):
            tris = ds.soup(n, n)
            nodes, idx = native.build_bvh(tris)
            rows = marked(tris[idx], n)
            ctx.upload_scene(nodes if fl & 3 else None, rows, mats)
            got = ctx.read_triangles()
            assert got.dtype == np.float32 and same(got, rows), (n, first_row(got, rows))
            into = np.zeros((n, 16), np.float32)
            assert ctx.read_triangles_into(into) is into and same(into, rows)
            dev = torch_rows(n)
            assert ctx.read_triangles_into(dev) is dev
            assert same(dev.cpu().numpy(), rows), (n, "device")
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def cornell():
    from rvpt_amd import scene
    tris, mats = scene.cornell_scene(2)
    assert tris.shape[0] == 2300
    tris = marked(tris[np.random.RandomState(2).permutation(tris.shape[0])], 23)
    tris[:, 12] = scene.cornell_scene(2)[0][np.random.RandomState(2).permutation(2300), 12]  # (the materials the scene means)
    tris.setflags(write=False)
    return tris, mats


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_a_build_reads_back_in_the_callers_order(native, cornell, method):
    """Case 2.  build_scene of 2 300 shuffled triangles: every builder stores another order, the read is the caller's array — hence the three are equal."""
    tris, mats = cornell
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, method) == method
        got = ctx.read_triangles()
        assert same(got, tris), first_row(got, tris)
        dev = ctx.read_triangles_into(torch_rows(2300))
        assert same(dev.cpu().numpy(), tris)
    finally:
        ctx.close()


@pytest.mark.parametrize("seed,source", [(13, "brute"), (3, "lbvh"), (4, "ploc"), (5, "sah")])
def test_every_step_of_a_sequence_reads_back_the_models_rows(native, seed, source):
    """Case 3.  Four of tests/_scene_model.py's seeded sequences (SUITE's seeds for these sources) on a laboratory context: after EVERY step — refusals
    included — read_triangles() is Model.current byte for byte; every fourth step the same into a device tensor, with the laboratory read-back taken before
    and after the reads identical in every piece and flag."""
    steps = sm.sequence(seed, source, sm.MAX_STEPS)
    mats = sm.scene_of(sm.SCENE_NAMES[seed % len(sm.SCENE_NAMES)])[1]
    bvh = steps[0].args[0] is not None
    assert bvh == (source != "brute")
    model = sm.Model(bvh=bvh)
    ctx = native.Context(fu.W, fu.H, 0, 0, 1, native.TRAVERSAL_BVH if bvh else native.TRAVERSAL_BRUTE, lab=True)
    kinds = set()
    try:
        for i, step in enumerate(steps):
            what = f"step {i} ({step.kind})"
            try:
                fu.call(ctx, step, mats)
                refused = False
            except native.NativeError:
                refused = True
            try:
                sm.apply(model, step)
                model_refused = False
            except sm.Refused:
                model_refused = True
            assert refused == model_refused == step.refusal, what
            kinds.add(step.kind)
            before = ctx.scene_state(None if bvh else fu.BRUTE_PIECES) if i % 4 == 3 else None
            got = ctx.read_triangles()
            assert same(got, model.current), (what, first_row(got, model.current))
            if before is not None:
                dev = ctx.read_triangles_into(torch_rows(model.n))
                assert same(dev.cpu().numpy(), model.current), (what, "device")
                assert fu.same_states(before, ctx.scene_state(None if bvh else fu.BRUTE_PIECES)) is None, what
    finally:
        ctx.close()
    assert len(kinds) >= 6, kinds


def test_the_triangle_read_refuses_and_leaves_dst_alone(native, default_scene):
    """Case 4.  No scene; need - 1 bytes (RVPT_HIP_ERR_SIZE, both numbers); a device view 4 bytes in; dst poisoned beforehand and untouched every time; 64
    spare bytes past the end untouched on success, host and device; the empty scene is a no-op and takes NULL."""
    import torch
    tris, mats, nodes = default_scene
    n = tris.shape[0]
    need = n * 64
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        buf = np.full(need + 64, POISON, np.uint8)
        ptr = buf.ctypes.data_as(ctypes.c_void_p)
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, ptr, buf.nbytes)
        said = ctx._L.rvpt_hip_last_error(ctx._h)
        assert rc == native.ERR_INVALID and b"triangle read before any full upload_scene" in said and (buf == POISON).all()
        with pytest.raises(native.NativeError, match="before any full upload_scene") as e:
            ctx.read_triangles()
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, ptr, need - 1)
        said = ctx._L.rvpt_hip_last_error(ctx._h).decode()
        assert rc == native.ERR_SIZE and str(need - 1) in said and str(need) in said and (buf == POISON).all()
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, None, need)
        assert rc == native.ERR_INVALID and b"dst is NULL" in ctx._L.rvpt_hip_last_error(ctx._h)
        dev = torch.full((need + 64 + 16,), POISON, dtype=torch.uint8, device="cuda:0")
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, ctypes.c_void_p(dev.data_ptr() + 4), need)
        assert rc == native.ERR_INVALID and b"16-byte alignment" in ctx._L.rvpt_hip_last_error(ctx._h)
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, ctypes.c_void_p(dev.data_ptr()), need - 1)
        assert rc == native.ERR_SIZE
        assert bool((dev == POISON).all())
        # success: more than is needed is allowed, and what lies past the rows stays
        assert ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, ptr, buf.nbytes) == 0
        assert buf[:need].tobytes() == tris.tobytes() and (buf[need:] == POISON).all()
        assert b"dst holds" in ctx._L.rvpt_hip_last_error(ctx._h)  # a successful read leaves last_error as it was
        assert ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, ctypes.c_void_p(dev.data_ptr()), need + 64) == 0
        back = dev.cpu().numpy()
        assert back[:need].tobytes() == tris.tobytes() and (back[need:] == POISON).all()
        more = np.full((n + 1, 16), np.float32(7.5))
        ctx.read_triangles_into(more)
        assert same(more[:n], tris) and (more[n] == 7.5).all()
        # the empty scene
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        assert ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, None, 0) == 0
        buf[:] = POISON
        assert ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_TRIANGLES, ptr, buf.nbytes) == 0 and (buf == POISON).all()
        assert ctx.read_triangles().shape == (0, 16)
        # every other value is still the unknown format of a frame read
        for fmt in (7, 15, 26, 27, 77):
            rc = ctx._L.rvpt_hip_read(ctx._h, fmt, ptr, buf.nbytes)
            assert rc == native.ERR_INVALID and f"unknown format {fmt}".encode() in ctx._L.rvpt_hip_last_error(ctx._h) and (buf == POISON).all()
    finally:
        ctx.close()


def test_round_trips(native):
    """Case 5.  bind + skin on a SAH-built context.  Passing the read straight to the plain update form moves nothing: the next read and the next frames are
    the same.  A fresh context given build_scene(read, mats, "sah") holds numpy_tree("sah", model.current) — the tree Model._rebuild states for a guarded
    rebuild — by the laboratory read-back, and renders the frames an ordinary upload of that tree renders."""
    from rvpt_amd import scene
    tris, mats = sm.scene_of("default143")
    rec, bones = _skin.weights(tris, 6), _skin.bones(tris, 6, 0.4)
    model = sm.Model()
    model.build("sah", tris)
    model.bind(rec)
    model.skin(bones)
    cam = fu.camera_for(model.current)
    flags = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(fu.W, fu.H, 0, 0, 1, flags, lab=True)
    try:
        assert ctx.build_scene(tris, mats, "sah") == "sah"
        ctx.bind_skin(rec)
        ctx.skin(bones)
        read = ctx.read_triangles()
        assert same(read, model.current) and same(read, scene.skin_triangles(tris, rec, bones)) and not same(read, tris)
        frame = fu.frames(ctx, cam)
        ctx.update_triangles(read)
        model.update(read)
        assert same(ctx.read_triangles(), read)
        assert not model.differences(ctx.scene_state())
        assert same(fu.frames(ctx, cam), frame)
    finally:
        ctx.close()
    rebuilt = model.copy()
    rebuilt._rebuild()
    fresh_model = sm.Model()
    fresh_model.build("sah", read)
    assert same(fresh_model.nodes, rebuilt.nodes) and same(fresh_model.perm, rebuilt.perm)
    images = []
    for build in (True, False):
        fresh = native.Context(fu.W, fu.H, 0, 0, 1, flags, lab=True)
        try:
            if build:
                assert fresh.build_scene(read, mats, "sah") == "sah"
                assert not fresh_model.differences(fresh.scene_state())
                assert same(fresh.read_triangles(), read)
            else:
                fresh.upload_scene(fresh_model.nodes, fresh_model.stored(), mats)
            images.append(fu.frames(fresh, cam))
        finally:
            fresh.close()
    assert same(images[0], images[1])


# ---- format 6 ----------------------------------------------------------------------------------------------------------------------------------------------------

def poisoned(records):
    rec = records.copy()
    for name in ("point", "mat", "normal", "reserved"):
        rec[name].view(np.uint32)[...] = 0xCDCDCDCD
    return rec


def records_for(tris, seed, total):
    """SURFACE_POINT_DTYPE[total]: four invalid records first (prim = n and 0xFFFFFFFF, a NaN u, an infinite v), then every triangle at (0, 0), (1, 0), (0, 1)
    and the centroid, random interior pairs and pairs outside [0, 1] on random triangles; flags carry a pattern; the out fields are poisoned"""
    from rvpt_amd import native
    n = tris.shape[0]
    rng = np.random.RandomState(seed)
    rec = np.zeros(total, dtype=native.SURFACE_POINT_DTYPE)
    corners = np.array([(0, 0), (1, 0), (0, 1), (1 / 3, 1 / 3)], dtype=np.float32)
    k = 4 + 4 * n
    assert total >= k + 16
    rec["prim"][:4], rec["u"][:4], rec["v"][:4] = [n, NO_PRIM, 0, n - 1], [0.25, 0.25, np.nan, 0.5], [0.25, 0.25, 0.5, np.inf]
    rec["prim"][4:k] = np.repeat(np.arange(n, dtype=np.uint32), 4)
    rec["u"][4:k], rec["v"][4:k] = np.tile(corners[:, 0], n), np.tile(corners[:, 1], n)
    rest = total - k
    rec["prim"][k:] = rng.randint(0, n, rest)
    u = rng.uniform(0, 1, rest)
    v = rng.uniform(0, 1, rest) * (1 - u)
    outside = np.arange(rest) % 3 == 2
    u[outside], v[outside] = rng.uniform(-3, 3, outside.sum()), rng.uniform(-3, 3, outside.sum())
    rec["u"][k:], rec["v"][k:] = u, v
    rec["prim"][-3:], rec["u"][-3:], rec["v"][-3:] = [n + 7, 5, 6], [0.5, -np.inf, 0.5], [0.5, 0.5, np.nan]
    rec["flags"] = rng.randint(0, 2 ** 32, total, dtype=np.uint64).astype(np.uint32)
    return poisoned(rec)


def answer(tris, records):
    """the statement's records for `records`, whole: the in fields as given (flags included)"""
    from rvpt_amd import scene
    want = scene.surface_points(tris, records["prim"], records["u"], records["v"])
    want["flags"] = records["flags"]
    assert same(want["prim"], records["prim"]) and same(want["u"], records["u"]) and same(want["v"], records["v"])
    return want


def check(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and same(got, want), f"{what}: {first_row(got, want)}"


def device_records(records):
    import torch
    return torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12)).to("cuda:0")


def from_device(t, native):
    return t.cpu().numpy().view(native.SURFACE_POINT_DTYPE).reshape(-1)


@pytest.fixture(scope="module")
def record_set(default_scene):
    """(records, the statement's answer) on the default scene's 143 triangles in stored order, 64 k + 1 records.  Computed once, never changed."""
    tris = default_scene[0]
    assert tris.shape[0] == 143
    records = records_for(tris, 3, 65537)
    want = answer(tris, records)
    invalid = want["mat"] == NO_PRIM
    assert invalid[:4].all() and invalid[-3:].all() and invalid.sum() == 7 and np.isfinite(want["point"]).all() and np.isfinite(want["normal"]).all()
    records.setflags(write=False)
    want.setflags(write=False)
    return records, want


@pytest.mark.parametrize("kind", KINDS)
def test_surface_records_are_the_statements(native, default_scene, record_set, kind):
    """Case 6.  Whole records on every kind of context, from host arrays and from device tensors: batches of 1, 63, 64, 65, 257 (a work-group's 256 lanes and
    their tails) and 64 k + 1; every triangle at its corners and centroid, interior pairs, pairs outside [0, 1], the invalid records."""
    records, want = record_set
    tris, mats, nodes = default_scene
    fl = flags_of(native, kind)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
        for n in (1, 63, 64, 65, 257, 65537):
            for first in sorted({0, 4, records.shape[0] - n}):
                sub, sub_want = records[first:first + n], want[first:first + n]
                check(ctx.surface_points_into(sub.copy()), sub_want, f"{kind}, {n} host records from {first}")
                dev = device_records(sub)
                assert ctx.surface_points_into(dev) is dev
                check(from_device(dev, native), sub_want, f"{kind}, {n} device records from {first}")
        host_t = device_records(records[:300]).cpu()  # a host tensor goes the host way
        ctx.surface_points_into(host_t)
        check(host_t.numpy().view(native.SURFACE_POINT_DTYPE).reshape(-1), want[:300], "host tensor")
        out = ctx.surface_points(records["prim"][:700], records["u"][:700], records["v"][:700])  # the wrapper that makes the records: flags 0
        assert same(out["point"], want["point"][:700]) and same(out["normal"], want["normal"][:700]) and same(out["mat"], want["mat"][:700]) and (out["flags"] == 0).all()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def cornell_records(cornell):
    tris = cornell[0]
    records = records_for(tris, 29, 4 + 4 * 2300 + 3000)
    return records, answer(tris, records)


def test_prim_is_the_callers_index_after_every_builder(native, cornell, cornell_records):
    """Case 7.  After the three builders on 2 300 shuffled triangles: the same bytes, the statement's on the caller's array; the laboratory flags of the update
    forms' inverse permutation stay as they were (the read keeps an inverse of its own)."""
    tris, mats = cornell
    records, want = cornell_records
    answers = []
    for method in ("lbvh", "ploc", "sah"):
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
        try:
            assert ctx.build_scene(tris, mats, method) == method
            before = ctx.scene_state()
            assert before["have_perm"] and not before["have_inv_perm"]
            got = ctx.surface_points_into(records.copy())
            check(got, want, method)
            check(from_device(ctx.surface_points_into(device_records(records)), native), want, method + ", device records")
            assert fu.same_states(before, ctx.scene_state()) is None
            answers.append(got.tobytes())
        finally:
            ctx.close()
    assert answers[0] == answers[1] == answers[2]


@pytest.mark.parametrize("form", ["sparse", "pose", "guarded pose", "skin"])
@pytest.mark.parametrize("traversal", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_surface_records_follow_the_mesh_as_the_last_update_left_it(native, traversal, form):
    """Case 8.  After update_triangles(indices=), pose_parts, a guarded pose update that rebuilds (the permutation is replaced: the read's inverse must be made
    again) and bind_skin + skin: the statement on the update form's own numpy statement, in the caller's order.  The same records before and after: a point
    kept from frame to frame stays attached to the moved surface."""
    from rvpt_amd import scene
    tris, mats = scene.default_scene()
    n = tris.shape[0]
    records = records_for(tris, 19, 4 + 4 * n + 500)
    ctx = native.Context(64, 36, 0, 0, 1, getattr(native, traversal))
    try:
        assert ctx.build_scene(tris, mats, "lbvh") == "lbvh"
        before = ctx.surface_points_into(records.copy())
        check(before, answer(tris, records), f"{form}: before")
        if form == "sparse":
            idx = np.random.RandomState(7).permutation(n)[:n // 3]
            moved = tris.copy()
            moved[idx, :12] = scene.wobble(tris, 1.9, 0.1 * sm.extent(tris))[idx, :12]
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
            moves = [gp.turned(tris, f, c, 90.0)]  # (tests/test_nearest.py: the posed tree costs 1.050 of the built one)
            step = gp.step(gp.built(tris, "lbvh"), moves, 1.02, "lbvh")
            assert step.rebuilt
            moved = step.state.current
            report = ctx.pose_parts(moves, rebuild_above=1.02)
            assert report is None if traversal == "TRAVERSAL_BRUTE" else report.rebuilt
        got = ctx.surface_points_into(records.copy())
        rows = ctx.read_triangles()
    finally:
        ctx.close()
    assert same(rows, moved)
    check(got, answer(moved, records), form)
    assert not same(got, before)


@pytest.mark.parametrize("traversal", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_query_answers_pipe_straight_in(native, oracle, default_scene, traversal):
    """Case 9.  closest_points records fed in through their last quad (prim, u, v, region as the ignored flags word): whole records against the statement, and
    the point is `closest` bit for bit wherever the nearest form's clamp did nothing.  trace_rays hits, misses included, likewise."""
    tris, mats, nodes = default_scene
    fl = getattr(native, traversal)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
        points = ctx.closest_points_into(nq.base_points(tris, 31, counts=(600, 80, 80, 80, 40)))
        quads = np.ascontiguousarray(points.view(np.uint32).reshape(-1, 12)[:, 8:12])
        records = np.zeros(points.shape[0], dtype=native.SURFACE_POINT_DTYPE)
        records.view(np.uint32).reshape(-1, 12)[:, 0:4] = quads
        records = poisoned(records)
        assert same(records["prim"], points["prim"]) and same(records["u"], points["u"]) and same(records["flags"], points["region"])
        got = ctx.surface_points_into(records.copy())
        check(got, answer(tris, records), "piped point hits")
        hit = points["prim"] != NO_PRIM
        assert hit.sum() * 2 > points.shape[0]
        v = tris[points["prim"][hit]].reshape(-1, 4, 4)[:, :3, :3]
        lo, hi = v.min(axis=1), v.max(axis=1)
        inside = ((got["point"][hit] >= lo) & (got["point"][hit] <= hi)).all(axis=1)  # the clamp q < lo ? lo : (q > hi ? hi : q) did nothing
        assert inside.sum() * 4 > hit.sum() and same(got["point"][hit][inside], points["closest"][hit][inside])
        rays = rq.base_rays(tris, 37, counts=(200, 200, 60, 60, 60, 40))
        hits = ctx.trace_rays_into(rays.copy())
        assert (hits["prim"] != NO_PRIM).sum() > 100 and (hits["prim"] == NO_PRIM).any()
        piped = ctx.surface_points(hits["prim"], hits["u"], hits["v"])
        want = answer(tris, piped)
        check(piped, want, "piped ray hits")
        struck = hits["prim"] != NO_PRIM
        along = hits["org"][struck].astype(np.float64) + hits["t"][struck].astype(np.float64)[:, None] * hits["dir"][struck].astype(np.float64)
        assert np.abs(piped["point"][struck] - along).max() < 1e-3 * sm.extent(tris)  # (NOT org + t*dir bit for bit, but the same place)
    finally:
        ctx.close()


def probe_rays(tris):
    """one ray per triangle: from centroid + 1e-3 extent n along -n, tmax 4e-3 extent (float64, rounded once)"""
    v = tris.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    ext = sm.extent(tris)
    return (v.mean(axis=1) + 1e-3 * ext * nrm).astype(np.float32), (-nrm).astype(np.float32), np.float32(4e-3 * ext)


@pytest.mark.parametrize("which", ["default", "cornell1"])
@pytest.mark.parametrize("upload", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE", "sah"])
def test_the_normal_is_the_path_tracers(native, which, upload):
    """Case 10.  For every triangle a short ray onto its own centroid: trace_rays must report that very triangle for EVERY ray (checked beforehand on the CPU
    with _ray_query.Statement in the brute-force order, the host builder's leaf order and the LBVH and SAH builders' orders: 143 of 143 and 584 of 584), and
    trace_paths(mode=3)'s radiance is fmaf(0.5, normal, 0.5) of the surface record, bit for bit.  After a skin update (six bones of _skin.bones at phase 0.4:
    143 of 143 and 582 of 584 on the CPU) at least nine tenths report their own triangle, and those are compared."""
    from rvpt_amd import scene
    tris, mats = scene.default_scene() if which == "default" else scene.cornell_scene(1)
    n = tris.shape[0]
    assert n == (143 if which == "default" else 584)
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH if upload == "sah" else getattr(native, upload))
    try:
        if upload == "sah":
            assert ctx.build_scene(tris, mats, "sah") == "sah"
        else:
            nodes, idx = native.build_bvh(tris)
            tris = np.ascontiguousarray(tris[idx])
            ctx.upload_scene(nodes if upload == "TRAVERSAL_BVH" else None, tris, mats)
        for skinned in (False, True):
            if skinned:
                rec, bones = _skin.weights(tris, 6), _skin.bones(tris, 6, 0.4)
                ctx.bind_skin(rec)
                ctx.skin(bones)
                now = scene.skin_triangles(tris, rec, bones)
                assert same(ctx.read_triangles(), now)
            else:
                now = tris
            org, dirv, tmax = probe_rays(now)
            hits = ctx.trace_rays(org, dirv, tmax)
            own = hits["prim"] == np.arange(n)
            assert own.sum() * 10 >= 9 * n if skinned else own.all(), (which, upload, skinned, int(own.sum()))
            surf = ctx.surface_points(hits["prim"], hits["u"], hits["v"])
            check(surf, answer(now, surf), f"{which}, {upload}, skinned {skinned}")
            paths = ctx.trace_paths(org, dirv, np.arange(n, dtype=np.uint32), 1, mode=3)
            want = scene._fmaf(np.float32(0.5), surf["normal"][own], np.float32(0.5))
            assert same(paths["radiance"][own], want), first_row(paths["radiance"][own], want)
            assert same(surf["normal"][own], scene.triangle_unit_normals(now)[own])
    finally:
        ctx.close()


def test_the_reads_leave_the_rest_alone(native, default_scene, record_set):
    """Case 11.  47 and 49 bytes, a misaligned tensor, no scene, the empty scene: INVALID in a ray query's words, memory untouched.  Two accumulated frames,
    both reads, a third frame: image, stats, the timing's dispatch count, launch_info, cull_info and last_error equal a context that never read."""
    import torch
    from rvpt_amd import RenderSettings
    records, want = record_set
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        host12 = torch.from_numpy(records[:64].copy().view(np.float32).reshape(-1, 12))
        with pytest.raises(native.NativeError, match="surface query before any full upload_scene.*no scene to ask") as e:
            ctx.surface_points_into(host12.clone())
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        flat = host12.to("cuda:0").reshape(-1)
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="surface records on the device need 16-byte alignment") as e:
            ctx.surface_points_into(flat[1:1 + 12 * 5].reshape(5, 12))
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        buf = records[:2].copy()
        for nbytes in (47, 49):
            rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_SURFACE_POINTS, buf.ctypes.data_as(ctypes.c_void_p), nbytes)
            said = ctx._L.rvpt_hip_last_error(ctx._h)
            assert rc == native.ERR_INVALID and b"surface query" in said and b"multiple" in said and b"rvpt_surface_point" in said
            assert buf.tobytes() == records[:2].tobytes()
        ctx.surface_points_into(records[:1].copy())  # a successful read leaves last_error as it was
        ctx.read_triangles()
        assert b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h)
        assert ctx.surface_points_into(records[:0].copy()).shape == (0,)
        assert ctx.surface_points_into(torch.zeros((0, 12), device="cuda:0")).shape == (0, 12)
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)  # the empty scene: every record is invalid, every out field written
        empty = ctx.surface_points_into(records[:300].copy())
        check(empty, answer(np.zeros((0, 16), np.float32), records[:300]), "the empty scene")
        assert (empty["mat"] == NO_PRIM).all()
    finally:
        ctx.close()
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for reads in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.build_scene(tris, mats, "sah")
            if reads:
                ctx.surface_points_into(records[:300].copy())  # before any set_frame
                ctx.read_triangles()
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if reads and f == 1:  # (with frames in flight: the calls wait for them)
                    ctx.surface_points_into(records[:5000].copy())
                    ctx.read_triangles_into(torch_rows(tris.shape[0]))
                    ctx.read_triangles()
            img = ctx.read()
            out.append((img.tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info(), ctx._L.rvpt_hip_last_error(ctx._h)))
        finally:
            ctx.close()
    assert out[0] == out[1]


def test_any_rank_of_a_partition_reads(native, default_scene, record_set):
    """tile_world = 2 without a communicator: rank 1's context holds the whole scene; both reads are local and return case 1's and case 6's bytes."""
    records, want = record_set
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 1, 2, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, tris, mats)
        check(ctx.surface_points_into(records[:3000].copy()), want[:3000], "rank 1 of 2")
        assert same(ctx.read_triangles(), tris)
    finally:
        ctx.close()


@pytest.mark.parametrize("traversal,build", [("bvh", "host"), ("brute", "host"), ("bvh", "device-sah")])
def test_rvpt_reads_in_the_order_triangles_were_added(native, traversal, build):
    """RVPT.read_triangles / RVPT.surface_points: rows and prim in the order the triangles were ADDED, through primitive_indices after a host build (the host
    builder reorders the 288 triangles), before and after a plain update; a trace_rays answer pipes straight in."""
    from rvpt_amd import RVPT, scene
    tris, mats = scene.heightfield_scene(cells=12)
    n = tris.shape[0]
    r = RVPT(64, 36, device=0, traversal=traversal, build=build)
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        if build == "host":
            assert not (np.asarray(r.primitive_indices) == np.arange(n)).all()
        assert same(r.read_triangles(), tris)
        moved = scene.wobble(tris, 0.7, 0.02 * sm.extent(tris))
        r.update_triangles(moved)
        assert same(r.read_triangles(), moved)
        out = np.zeros((n, 16), np.float32)
        assert r.read_triangles(out=out) is out and same(out, moved)
        prim = np.arange(n, dtype=np.uint32)[::-1].copy()
        u, v = np.full(n, 0.25, np.float32), np.full(n, 0.5, np.float32)
        got = r.surface_points(prim, u, v)
        want = scene.surface_points(moved, prim, u, v)
        check(got, want, "RVPT.surface_points")
        org, dirv, tmax = probe_rays(moved)
        hits = r.trace_rays(org, dirv, tmax)
        assert (hits["prim"] == np.arange(n)).all()
        piped = r.surface_points(hits)
        check(piped, scene.surface_points(moved, hits["prim"], hits["u"], hits["v"]), "RVPT.surface_points(hits)")
    finally:
        r.shutdown()
