"""Crossing queries on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_RAY_CROSSINGS (Context.count_crossings_into) against the statement of tests/_crossings.py.
Everything is bit-exact and whole records are compared byte for byte — the in fields must come back as sent; no ray is left out."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

import _crossings as cr
import _multi_hit as mh
import _ray_query as rq
from _util import identity_camera
from test_ray_query import kernel_constant
from test_refit import bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
KINDS = [("TRAVERSAL_BVH", 0), ("TRAVERSAL_BVH_ORDERED", 0), ("TRAVERSAL_BVH|BVH_PER_LANE", 0), ("TRAVERSAL_BRUTE", 1)]


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def flags_of(native, names):
    fl = 0
    for name in names.split("|"):
        fl |= getattr(native, name)
    return fl


def readonly(a):
    a.setflags(write=False)
    return a


def context(native, fl, scene3, lab=None, upload=None):
    ctx = native.Context(64, 36, 0, 0, 1, fl, lab=lab)
    try:
        if upload is not None:
            upload(ctx)
        else:
            tris, mats, nodes = scene3
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
    except BaseException:
        ctx.close()
        raise
    return ctx


def ask(ctx, records, want, what):
    got = ctx.count_crossings_into(records.copy())
    cr.check(got, want, records, what)
    return got


@pytest.fixture(scope="module")
def whole_set(oracle, default_scene):
    """{traversal: (records, answer)} for the 2048 + 37 rays of tests/test_ray_query.py, their tmax variants and a dozen non-finite records.  Computed once,
    read-only."""
    tris, _, nodes = default_scene
    st = cr.Statement(oracle, nodes, tris)
    base = rq.base_rays(tris, 7)
    assert base.shape[0] == 2048 + 37 and tris.shape[0] == 143
    rays = np.concatenate([rq.with_tmax_variants(base, st.answer(base)), rq.non_finite_records(base, 9, 12)])
    assert rays.shape[0] % 64 and rays.shape[0] % 256
    records = readonly(cr.records_of(rays))
    out = {traversal: (records, readonly(st.answer_crossings(records, traversal))) for traversal in (0, 1)}
    want = out[0][1]
    assert (want["front"] > 0).sum() > 1000 and (want["back"] > 0).sum() > 1000 and (want["front"] + want["back"] >= 3).sum() > 50
    assert not want["front"][-12:].any() and not want["back"][-12:].any()
    return out


@pytest.fixture(scope="module")
def answered(native, default_scene, whole_set):
    """what every kind of context answered for the whole set, filled by the test below as it goes: the three BVH kinds are then held against one another"""
    return {}


@pytest.mark.parametrize("flags,traversal", KINDS)
def test_the_default_scene_on_every_kind_of_context(native, default_scene, whole_set, answered, flags, traversal):
    records, want = whole_set[traversal]
    ctx = context(native, flags_of(native, flags), default_scene)
    try:
        got = ask(ctx, records, want, flags)
    finally:
        ctx.close()
    none = (got["front"] == 0) & (got["back"] == 0)
    assert (bits(got["t_near"][none]) == bits(got["tmax"][none])).all() and not bits(got["t_far"][none]).any()
    answered[flags] = got.tobytes()
    bvh = [answered[f] for f, t in KINDS if t == 0 and f in answered]
    assert all(b == bvh[0] for b in bvh)  # the answer does not depend on the visiting order


@pytest.fixture(scope="module")
def layered():
    """(the flipped layered scene in shuffled stored order, mats, 256 through rays, their reverses, the same with tmax between two layers and exactly on one)"""
    from rvpt_amd import scene
    tris, zs = cr.flipped_layered_scene()
    fwd = mh.through_rays(256, 23)
    back = cr.reversed_rays(fwd, 8.0)
    cut = np.concatenate([fwd[:64], fwd[:64]])
    layer_z = sorted(set(zs))
    dz = fwd["dir"][:64, 2].astype(np.float64)
    cut["tmax"][:64] = ((layer_z[3] + layer_z[4]) / 2 / dz).astype(np.float32)  # between the fourth and the fifth distinct layer
    return tris, scene.default_materials(), readonly(cr.records_of(np.concatenate([fwd, back, cut]))), (zs[::2], layer_z[3])


def layered_answer(oracle, nodes, stored, records, layers):
    st = cr.Statement(oracle, nodes, stored)
    traversal = 1 if nodes is None else 0
    rec = records.copy()
    # the last 64: tmax exactly at the t the statement gives the ray's fourth distinct layer
    for j in range(64):
        r = rec[-64 + j]
        ts = sorted(set(h[1] for h in st.trace_k(r["org"], r["dir"], cr.NO_LIMIT, np.inf, True, traversal)))
        rec["tmax"][-64 + j] = ts[3]
    want = st.answer_crossings(rec, traversal)
    total = want["front"].astype(np.int64) + want["back"]
    assert (total[:512] == mh.LAYERS).all() and (want["front"][:512] > 0).all() and (want["back"][:512] > 0).all()  # 12, the duplicates counted, split by facing
    assert (want["front"][256:512] == want["back"][:256]).all()
    z, z_cut = layers  # up to and with the fourth distinct layer, duplicates counted; the strict test drops every copy of the layer that lies on tmax
    assert (z <= z_cut).sum() == 7 and (z < z_cut).sum() == 4 and (total[512:576] == 7).all() and (total[576:] == 4).all()
    return rec, want


@pytest.mark.parametrize("how", ["brute", "host", "lbvh", "ploc", "sah"])
def test_the_flipped_layers(native, oracle, layered, how):
    """12 crossings split by facing on 256 through rays and their reverses, tmax between layers and exactly on a layer — on a brute-force context, over the
    host tree, and after each of the three device builders, where the stored order differs from the caller's"""
    from rvpt_amd import native as n, scene
    tris, mats, records, layers = layered
    if how == "brute":
        nodes, stored, fl, upload = None, tris, native.TRAVERSAL_BRUTE, lambda c: c.upload_scene(None, tris, mats)
    elif how == "host":
        nodes, idx = n.build_bvh(tris)
        stored = np.ascontiguousarray(tris[idx])
        fl, upload = native.TRAVERSAL_BVH, lambda c: c.upload_scene(nodes, stored, mats)
    else:
        nodes, perm = {"lbvh": scene.build_lbvh, "ploc": scene.build_ploc, "sah": scene.build_sah}[how](tris)[:2]
        stored = np.ascontiguousarray(tris[perm])
        assert not np.array_equal(np.asarray(perm), np.arange(tris.shape[0]))
        fl, upload = native.TRAVERSAL_BVH, lambda c: c.build_scene(tris, mats, how) == how or pytest.fail("fell back")
    rec, want = layered_answer(oracle, nodes, stored, records, layers)
    ctx = context(native, fl, None, upload=upload)
    try:
        ask(ctx, rec, want, how)
    finally:
        ctx.close()


def test_after_a_skin_update_and_a_guarded_pose_that_rebuilds(native, oracle):
    """Against the statement over the model's tree (tests/_scene_model.py) with the POSED normals: after bind + skin (a refit), then after a guarded pose update
    past its limit (a rebuild: new tree, new permutation)"""
    import _guarded_pose as gp
    import _scene_model as sm
    import _skin
    tris, mats = sm.scene_of("default143")
    limit = 1.05
    model = sm.Model()
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, "sah") == "sah"
        model.build("sah", tris)
        rest_normals = cr.Statement(oracle, model.nodes, model.stored()).unit_n.tobytes()
        rec, m = _skin.weights(tris, 7), _skin.bones(tris, 7)
        ctx.bind_skin(rec)
        ctx.skin(m)
        model.bind(rec)
        model.skin(m)
        seen = []
        for step in ("skin", "pose"):
            if step == "pose":
                f, c = gp.part_of(model.n)
                moves = [gp.turned(model.rest, f, c, 90.0)]
                report = model.pose_guarded(moves, limit)
                assert report.rebuilt
                assert ctx.pose_parts(moves, rebuild_above=limit).rebuilt
            records = cr.records_of(rq.base_rays(model.current, 19, counts=(80, 160, 40, 60, 60, 21)))
            st = cr.Statement(oracle, model.nodes, model.stored())
            assert st.unit_n.tobytes() != rest_normals
            want = st.answer_crossings(records)
            assert (want["front"] > 0).sum() > 100 and (want["back"] > 0).sum() > 100
            ask(ctx, records, want, f"after {step}")
            seen.append(model.current.tobytes())
        assert seen[0] != seen[1]
    finally:
        ctx.close()


def test_a_deep_tree(native, oracle):
    """Rays down the 37-level tree "sah" makes of tests/_device_state.py's hittable ladder, past the kQueryLdsLevels = 8 slots a lane keeps in LDS: one ray over
    every triangle with tmax = 8 h, 64 more past every triangle"""
    import _device_state as ds
    from rvpt_amd import scene
    assert kernel_constant("kQueryLdsLevels") == 8
    h = ds.HITTABLE_LADDER["h"]
    tris = ds.ladder(**ds.HITTABLE_LADDER)
    mats = scene.default_materials()
    n = tris.shape[0]
    nodes, perm, _ = scene.build_sah(tris)
    centroid = ds.vertices(tris).astype(np.float64).mean(axis=1)
    org = np.concatenate([centroid + [0.0, 4.0 * h, 0.0], centroid[:64] + [0.0, 4.0 * h, 3.0 * h]])
    records = cr.make_records(org, np.tile([0.0, -1.0, 0.0], (n + 64, 1)), np.float32(8.0 * h))
    want = cr.Statement(oracle, nodes, tris[perm]).answer_crossings(records)
    total = want["front"].astype(np.int64) + want["back"]
    assert 4 * int((total[:n] > 0).sum()) >= 3 * n and (total[:n] > 1).any() and not total[n:].any()
    ctx = context(native, native.TRAVERSAL_BVH, None, lab=True, upload=lambda c: c.build_scene(tris, mats, "sah") == "sah" or pytest.fail("fell back"))
    try:
        state = ctx.scene_state(pieces=[])
        assert state["bvh_height"] == 37 and state["n_wide"] > 0
        ask(ctx, records, want, "ladder, sah")
    finally:
        ctx.close()


def test_the_binary_walk(native, oracle, default_scene, whole_set, monkeypatch):
    """The laboratory build with the caller-layout knob holds no wide form: walk_bvh2<Crossings> on 600 records of the whole set"""
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    records, want = whole_set[0]
    ctx = context(native, native.TRAVERSAL_BVH, default_scene, lab=True)
    try:
        state = ctx.scene_state(pieces=[])
        assert state["n_wide"] == 0 and state["bvh_height"] > 0
        ask(ctx, records[1800:2400], want[1800:2400], "binary walk")
    finally:
        ctx.close()


def test_brute_force_tiles(native, oracle):
    """Cornell + 9 k (9164 triangles: seventeen LDS tiles and a tail) with 64 rays on a brute-force context; the same 64 rays on a BVH context are held against
    the BVH statement"""
    from rvpt_amd import native as n, scene
    tile = kernel_constant("kQueryTileTris")
    tris, mats = scene.cornell_scene()
    assert tile == 512 and tris.shape[0] > 17 * tile and tris.shape[0] % tile
    records = cr.records_of(rq.base_rays(tris, 13, counts=(24, 24, 4, 4, 4, 4)))
    assert records.shape[0] == 64
    want = cr.Statement(oracle, None, tris).answer_crossings(records, 1)
    assert (want["front"] + want["back"] >= 2).sum() > 20
    ctx = context(native, native.TRAVERSAL_BRUTE, (tris, mats, None))
    try:
        ask(ctx, records, want, "brute force, eighteen tiles")
    finally:
        ctx.close()
    nodes, idx = n.build_bvh(tris)
    stored = np.ascontiguousarray(tris[idx])
    want = cr.Statement(oracle, nodes, stored).answer_crossings(records, 0)
    ctx = context(native, native.TRAVERSAL_BVH, (stored, mats, nodes))
    try:
        ask(ctx, records, want, "the same rays over the tree")
    finally:
        ctx.close()


@pytest.mark.parametrize("flags,traversal", [KINDS[0], KINDS[3]])
def test_relations_to_the_queries_that_exist(native, default_scene, whole_set, flags, traversal):
    """Where front + back <= 8 the non-miss slots of an any-hit k = 8 query are that many, and their min and max t are t_near and t_far; on the brute-force
    context t_near equals format 2's t"""
    records, want = whole_set[traversal]
    records = records[:2085 + 600]
    ctx = context(native, flags_of(native, flags), default_scene)
    try:
        got = ctx.count_crossings_into(records.copy())
        rays = records.copy().view(native.RAY_HIT_DTYPE)
        rays["flags"] = native.RAY_ANY_HIT
        lists = ctx.trace_rays_into(mh.groups(rays, 8), hits=8).reshape(-1, 8)
        held = lists["prim"] != mh.NO_PRIM
        total = got["front"].astype(np.int64) + got["back"]
        short = total <= 8
        assert short.sum() > 2000 and (held.sum(axis=1)[short] == total[short]).all() and (held.sum(axis=1)[~short] == 8).all()
        some = short & (total > 0)
        t = np.where(held, lists["t"], np.nan)
        assert (bits(np.nanmin(t[some], axis=1)) == bits(got["t_near"][some])).all() and (bits(np.nanmax(t[some], axis=1)) == bits(got["t_far"][some])).all()
        if traversal == 1:
            rays["flags"] = 0
            closest = ctx.trace_rays_into(rq.poisoned(rays))
            assert (bits(closest["t"]) == bits(got["t_near"])).all() and ((closest["prim"] == mh.NO_PRIM) == (total == 0)).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("flags,traversal", [KINDS[0], KINDS[3]])
def test_batches_and_memory(native, default_scene, whole_set, flags, traversal):
    """1, 63, 64, 65 and 257 records — the run boundaries of the claim, a last wave that is partly live — and nothing past the last record is written; host
    numpy records, a host tensor and a device tensor give the same bytes; the any-hit bit changes nothing"""
    import torch
    records, want = whole_set[traversal]
    ctx = context(native, flags_of(native, flags), default_scene)
    try:
        for n in (1, 63, 64, 65, 257):
            buf = np.concatenate([records[:n], records[:2]])  # a tail the call is not given
            got = ctx.count_crossings_into(buf[:n])
            cr.check(got, want[:n], records[:n], f"{flags} n={n}")
            assert (buf[n:].view(np.uint32).reshape(-1, 12)[:, 8:] == cr.POISON).all()
        part, part_want = records[:1000], want[:1000]
        host12 = torch.from_numpy(part.copy().view(np.float32).reshape(-1, 12))
        host_t = host12.clone()
        assert ctx.count_crossings_into(host_t) is host_t
        cr.check(host_t.numpy().view(native.RAY_CROSSINGS_DTYPE).reshape(-1), part_want, part, "host tensor")
        dev = host12.to("cuda:0")
        assert ctx.count_crossings_into(dev) is dev
        cr.check(dev.cpu().numpy().view(native.RAY_CROSSINGS_DTYPE).reshape(-1), part_want, part, "device records")
        assert (part["flags"] & 1).sum() > 300
        other = part.copy()
        other["flags"] ^= native.RAY_ANY_HIT
        got = ctx.count_crossings_into(other.copy())
        for name in cr.OUT:
            assert got[name].tobytes() == part_want[name].tobytes(), name
        wrapped = ctx.count_crossings(part["org"][:50], part["dir"][:50], part["tmax"][:50])
        for name in cr.OUT:
            assert wrapped[name].tobytes() == part_want[name][:50].tobytes(), name
    finally:
        ctx.close()


def test_refusals_and_the_empty_scene(native, default_scene, whole_set):
    import torch
    records, want = whole_set[0]
    records = records[:40].copy()
    tris, mats, nodes = default_scene
    read = lambda c, fmt, buf, nbytes: c._L.rvpt_hip_read(c._h, fmt, buf.ctypes.data_as(ctypes.c_void_p), nbytes)
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        buf = records.copy()
        with pytest.raises(native.NativeError, match="crossing query before any full upload_scene.*no scene to ask") as e:  # before any scene
            ctx.count_crossings_into(buf)
        assert e.value.code == native.ERR_INVALID and buf.tobytes() == records.tobytes()
        ctx.upload_scene(nodes, tris, mats)
        assert read(ctx, native.FORMAT_RAY_CROSSINGS, buf, 48 * 7 + 47) == native.ERR_INVALID  # not a multiple of 48
        said = ctx._L.rvpt_hip_last_error(ctx._h)
        assert b"crossing query" in said and b"383" in said and b"multiple" in said and b"rvpt_ray_crossings" in said and buf.tobytes() == records.tobytes()
        flat = torch.from_numpy(records.copy().view(np.float32).reshape(-1)).to("cuda:0")  # a device view that starts 4 bytes in
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="crossing records on the device need 16-byte alignment") as e:
            ctx.count_crossings_into(flat[1:1 + 12 * 6].reshape(6, 12))
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        assert read(ctx, native.FORMAT_RAY_CROSSINGS, buf, 0) == 0 and buf.tobytes() == records.tobytes()  # a no-op
        assert ctx.count_crossings_into(records[:0].copy()).shape == (0,)
        for fmt in (7, 15, 26, 27, 32, 41, 48, 57, 77):  # still unknown, dst untouched
            assert read(ctx, fmt, buf, 48 * 6) == native.ERR_INVALID and b"unknown format %d" % fmt in ctx._L.rvpt_hip_last_error(ctx._h)
            assert buf.tobytes() == records.tobytes()
        ask(ctx, records, want[:40], "after the refusals")  # a successful query leaves last_error as it was
        assert b"unknown format 77" in ctx._L.rvpt_hip_last_error(ctx._h)
        # the empty scene: no crossing on any record, t_near carries tmax's bits, a NaN payload included
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        asked = records.copy()
        asked["tmax"].view(np.uint32)[::5] = 0x7FC12345
        empty = ctx.count_crossings_into(asked.copy())
        assert not empty["front"].any() and not empty["back"].any() and not bits(empty["t_far"]).any()
        assert (bits(empty["t_near"]) == bits(asked["tmax"])).all() and (bits(empty["t_near"][::5]) == 0x7FC12345).all()
        for name in ("org", "tmax", "dir", "flags"):
            assert empty[name].tobytes() == asked[name].tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_a_frame_stays_the_same(native, default_scene, whole_set, flags):
    """Two accumulated frames, a crossing query, a third frame: image, stats, the timing's dispatch count, launch_info, cull_info and last_error equal a context
    that never asked"""
    from rvpt_amd import RenderSettings
    records = whole_set[0][0][:1000]
    tris, mats, nodes = default_scene
    fl = getattr(native, flags) | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for asks in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
            if asks:
                ctx.count_crossings_into(records.copy())  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.count_crossings_into(records.copy())  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info(), bytes(ctx._L.rvpt_hip_last_error(ctx._h))))
        finally:
            ctx.close()
    assert out[0] == out[1]


def _renderer(tris, **kw):
    from rvpt_amd import RVPT, scene
    r = RVPT(64, 36, device=0, **kw)
    r.add_triangles(tris)
    for m in scene.default_materials():
        r.add_material(m)
    r.initialize()
    return r


@pytest.mark.parametrize("name", ["cube", "icosphere"])
@pytest.mark.parametrize("kw", [dict(traversal="bvh"), dict(traversal="bvh", build="device"), dict(traversal="brute")], ids=["host", "device", "brute"])
def test_inside_and_signed_distance(native, name, kw):
    """RVPT.inside under both rules against the known truth for 40 points inside and 40 outside (tests/test_crossings_host.py checks what the points must be),
    and RVPT.signed_distance against sqrt of scene.closest_points with that sign"""
    from rvpt_amd import scene
    from test_crossings_host import SHAPES, probe_points
    tris = SHAPES[name][0]()
    points, truth = probe_points(name)
    r = _renderer(tris, **kw)
    try:
        for rule in ("winding", "parity"):
            got = r.inside(points, rule=rule)
            assert got.dtype == bool and np.array_equal(got, truth), rule
        sd = r.signed_distance(points)
        want = np.sqrt(scene.closest_points(tris, points)["d2"])
        assert sd.dtype == np.float32 and sd.tobytes() == np.where(truth, -want, want).astype(np.float32).tobytes()
        odd = np.concatenate([points[:2], np.float32([[np.nan, 0, 0]])])
        assert r.inside(odd).tolist() == [True, True, False] and r.signed_distance(odd)[2] == np.inf
        rec = r.count_crossings(points[:3], [[0.3, 0.4, 0.5]] * 3)
        assert rec.dtype == native.RAY_CROSSINGS_DTYPE and (rec["back"] == 1).all() and (rec["front"] == 0).all()
    finally:
        r.shutdown()


@pytest.mark.parametrize("idx", [1, 3, 8, 13, 22, 35, 38, 43])
def test_hostile_scenes(native, oracle, idx):
    """Eight cases of the hostile fuzz's slice (tools/fuzz_bvh.py): slivers, duplicates and zero-area triangles, scales of 2^-20 .. 2^20.  The host tree and a
    device-built tree, each against the statement over that tree"""
    sys.path.insert(0, str(ROOT / "tools"))
    import fuzz_bvh
    case = fuzz_bvh.reduced_case(606, idx, 64, 36, max_tris=256)
    assert (case["kind"], case["k"]) == {1: ("slivers", 0), 3: ("soup_dup", 0), 8: ("soup_dup", -2), 13: ("soup_dup", -3), 22: ("model", -20), 35: ("slivers", -18),
                                         38: ("soup_dup", 18), 43: ("soup", 20)}[idx]
    with np.errstate(all="ignore"):
        records = cr.records_of(rq.base_rays(case["tris"], idx, counts=fuzz_bvh.RAY_COUNTS))
        trees = [t for t in fuzz_bvh.case_trees(case) if t["name"] != "loose"]
        assert [t["method"] for t in trees] == [None, fuzz_bvh.METHODS[idx % 3]]
        wants = [cr.Statement(oracle, t["nodes"], t["tris"]).answer_crossings(records) for t in trees]
    for tree, want in zip(trees, wants):
        ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
        try:
            fuzz_bvh.upload(ctx, case, tree)
            ask(ctx, records, want, f"case {idx}, {tree['name']}")
        finally:
            ctx.close()
