"""K-nearest ray queries on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k) (Context.trace_rays_into(records, hits=k)) against the statement of
tests/_multi_hit.py.  Everything is bit-exact and whole records are compared byte for byte — the followers' poisoned in fields and the first two quads of every
record included; no ray is left out."""
import ctypes

import numpy as np
import pytest

import _multi_hit as mh
import _ray_query as rq
from _util import identity_camera
from test_gpu_parity import _loosen_boxes
from test_ray_query import _mirrored_chain, kernel_constant
from test_refit import bits

pytestmark = pytest.mark.gpu

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


@pytest.fixture(scope="module")
def layered():
    """(tris in shuffled stored order, mats, nodes over them, tris in leaf order)"""
    from rvpt_amd import native as n, scene
    tris, _ = mh.layered_scene()
    nodes, idx = n.build_bvh(tris)
    return tris, scene.default_materials(), nodes, np.ascontiguousarray(tris[idx])


def layered_rays(tris):
    """about 300: 150 straight through every layer, 150 of every kind of base_rays; a third any hit"""
    rays = np.concatenate([mh.through_rays(150, 23), rq.base_rays(tris, 29, counts=(50, 50, 20, 10, 10, 10))])
    rays["flags"] = np.where(np.arange(rays.shape[0]) % 3 == 0, 1, 0)
    return rays


@pytest.fixture(scope="module")
def sweep(oracle, default_scene, layered):
    """{(scene, traversal, k): (records, the statement's answer)} for k = 1 .. 8 on about 300 rays of the default scene and of the layered scene.  Computed
    once, read-only."""
    tris, _, nodes = default_scene
    ltris, _, lnodes, lsorted = layered
    rays = {"default": rq.base_rays(tris, 31, counts=(90, 90, 40, 30, 30, 20)), "layered": layered_rays(ltris)}
    st = {("default", 0): mh.Statement(oracle, nodes, tris), ("default", 1): mh.Statement(oracle, None, tris),
          ("layered", 0): mh.Statement(oracle, lnodes, lsorted), ("layered", 1): mh.Statement(oracle, None, ltris)}
    out = {}
    for (name, traversal), s in st.items():
        for k in range(1, 9):
            records = mh.groups(rays[name], k)
            out[name, traversal, k] = (readonly(records), readonly(s.answer_k(records, k, traversal)))
    # what the sweep must reach: full lists, short lists, drops, equal t in neighbouring slots
    want = out["layered", 1, 8][1].reshape(-1, 8)
    assert (want["prim"][:, 7] != mh.NO_PRIM).sum() > 50 and ((want["prim"][:, 0] != mh.NO_PRIM) & (want["prim"][:, 7] == mh.NO_PRIM)).sum() > 10
    closest = (want["flags"][:, 0] & 1) == 0
    assert ((want["t"][:, 1] == want["t"][:, 2]) & (want["prim"][:, 2] != mh.NO_PRIM) & closest).sum() > 50
    return out


@pytest.fixture(scope="module")
def whole_set(oracle, default_scene):
    """{(traversal, k): (records, answer)} for k = 4 and 8 on the 2048 + 37 rays of tests/test_ray_query.py, their tmax variants and a dozen non-finite records"""
    tris, _, nodes = default_scene
    st = mh.Statement(oracle, nodes, tris)
    base = rq.base_rays(tris, 7)
    assert base.shape[0] == 2048 + 37
    rays = np.concatenate([rq.with_tmax_variants(base, st.answer(base)), rq.non_finite_records(base, 9, 12)])
    assert rays.shape[0] % 64 and rays.shape[0] % 256
    out = {}
    for k in (4, 8):
        records = readonly(mh.groups(rays, k))
        for traversal in (0, 1):
            out[traversal, k] = (records, readonly(st.answer_k(records, k, traversal)))
    assert not rq.same_bytes(out[0, 8][1], out[1, 8][1])  # the two orders do differ somewhere
    assert (out[0, 8][1].reshape(-1, 8)["prim"][-12:] == mh.NO_PRIM).all()
    return out


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


def ask(ctx, records, k, what):
    def check(want):
        got = ctx.trace_rays_into(records.copy(), hits=k)
        mh.check_groups(got, want, records, what)
        return got
    return check


@pytest.mark.parametrize("flags,traversal", KINDS)
def test_every_kind_of_context_answers_as_the_statement(native, default_scene, layered, sweep, flags, traversal):
    """k = 1 .. 8 on about 300 rays of the default scene and of the layered scene (insertion at every position, drops, equal t across slots)"""
    fl = flags_of(native, flags)
    ltris, lmats, lnodes, lsorted = layered
    for name, scene3 in (("default", default_scene), ("layered", (lsorted if traversal == 0 else ltris, lmats, lnodes))):
        ctx = context(native, fl, scene3)
        try:
            for k in range(1, 9):
                records, want = sweep[name, traversal, k]
                ask(ctx, records, k, f"{flags} {name} k={k}")(want)
        finally:
            ctx.close()


@pytest.mark.parametrize("flags,traversal", KINDS)
def test_the_whole_ray_set(native, default_scene, whole_set, flags, traversal):
    """k = 4 and 8 on the whole default ray set with its tmax variants and the non-finite records: those are k miss quads carrying tmax's bits"""
    ctx = context(native, flags_of(native, flags), default_scene)
    try:
        for k in (4, 8):
            records, want = whole_set[traversal, k]
            got = ask(ctx, records, k, f"{flags} k={k}")(want).reshape(-1, k)
            assert (got["prim"][-12:] == mh.NO_PRIM).all() and (bits(got["t"][-12:]) == bits(got["tmax"][-12:, :1])).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("flags,traversal", KINDS)
def test_k_1_is_format_2(native, default_scene, flags, traversal):
    """For the same records the out quads of format 33 are format 2's bytes, any-hit records, tmax variants and non-finite records included"""
    tris = default_scene[0]
    base = rq.base_rays(tris, 7)
    ctx = context(native, flags_of(native, flags), default_scene)
    try:
        first = ctx.trace_rays_into(base.copy())
        records = rq.poisoned(np.concatenate([rq.with_tmax_variants(base, first), rq.non_finite_records(base, 9, 12)]))
        two = ctx.trace_rays_into(records.copy())
        one = ctx.trace_rays_into(records.copy(), hits=1)
        assert (records["flags"] & 1).sum() > 500 and 500 < (two["prim"] != mh.NO_PRIM).sum()
        assert rq.same_bytes(one, two), rq.first_difference(one, two)
        assert rq.same_bytes(ctx.trace_rays_into(records.copy().reshape(-1, 1), hits=1).reshape(-1), two)
    finally:
        ctx.close()


def chain_scene():
    """48 triangles (24 quads along z) under the mirrored chain: every level leaves a leaf on the stack"""
    from rvpt_amd import scene
    rng = np.random.RandomState(11)
    quads = []
    for k in range(24):
        z, s, c = 1.0 + 0.25 * k, 0.3 + 0.05 * k, rng.uniform(-0.5, 0.5, 2)
        p = [(c[0] - s, c[1] - s, z), (c[0] + s, c[1] - s, z), (c[0] + s, c[1] + s, z), (c[0] - s, c[1] + s, z)]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    tris = scene.make_triangles(quads, 0)
    return tris, scene.default_materials(), _mirrored_chain(tris)


def test_the_binary_walk(native, oracle, default_scene, sweep, monkeypatch):
    """The laboratory build with the caller-layout knob holds no wide form: walk_bvh2<Nearest<CAP>>, every CAP, on the default scene and, past the 8 LDS levels,
    on the 48-level mirrored chain, at k = 3 and 8"""
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    ctx = context(native, native.TRAVERSAL_BVH, default_scene, lab=True)
    try:
        state = ctx.scene_state(pieces=[])
        assert state["n_wide"] == 0 and state["bvh_height"] > 0
        for k in (3, 8):
            records, want = sweep["default", 0, k]
            ask(ctx, records, k, f"binary walk k={k}")(want)
    finally:
        ctx.close()
    tris, mats, nodes = chain_scene()
    rays = rq.base_rays(tris, 5, counts=(60, 100, 40, 40, 40, 20))
    st = mh.Statement(oracle, nodes, tris)
    ctx = context(native, native.TRAVERSAL_BVH, (tris, mats, nodes), lab=True)
    try:
        state = ctx.scene_state(pieces=[])
        assert state["n_wide"] == 0 and state["bvh_height"] == 48 > kernel_constant("kQueryLdsLevels")
        for k in (3, 8):
            records = mh.groups(rays, k)
            want = st.answer_k(records, k)
            assert (want.reshape(-1, k)["prim"][:, k - 1] != mh.NO_PRIM).sum() > 20
            ask(ctx, records, k, f"binary walk, chain, k={k}")(want)
    finally:
        ctx.close()


@pytest.mark.parametrize("loose", [False, True])
@pytest.mark.parametrize("shape", ["ladder", "mirrored"])
def test_the_overflow_stack(native, oracle, shape, loose):
    """The wide walk past the kQueryLdsLevels = 8 slots a lane keeps in LDS, at k = 2 and 8: the 37-level tree "sah" makes of tests/_device_state.py's hittable
    ladder, uploaded as a caller's tree, and the 48-level mirrored chain (wide_stack_levels = 47); each tight and with loosened boxes.  A few hundred rays."""
    import _device_state as ds
    from rvpt_amd import scene
    lds_levels = kernel_constant("kQueryLdsLevels")
    assert lds_levels == 8
    if shape == "ladder":
        h = ds.HITTABLE_LADDER["h"]
        tris = ds.ladder(**ds.HITTABLE_LADDER)
        mats = scene.default_materials()
        nodes, perm, _ = scene.build_sah(tris)
        tris = np.ascontiguousarray(tris[perm])
        n = tris.shape[0]
        centroid = ds.vertices(tris).astype(np.float64).mean(axis=1)
        org = np.concatenate([centroid + [0.0, 4.0 * h, 0.0], centroid[:64] + [0.0, 4.0 * h, 3.0 * h]])
        flags = np.where(np.arange(n + 64) % 3 == 0, native.RAY_ANY_HIT, 0).astype(np.uint32)
        rays = rq.make_records(org, np.tile([0.0, -1.0, 0.0], (n + 64, 1)), np.float32(8.0 * h), flags)
    else:
        tris, mats, nodes = chain_scene()
        rays = rq.base_rays(tris, 3, counts=(60, 100, 40, 40, 40, 20))
    if loose:  # (the ladder's boxes span 2^101 down to 2^-32: a shrunk box on the way to the cluster culls every ray, so fewer of them are touched there)
        tight = nodes
        nodes = _loosen_boxes(nodes, 5, 0.1) if shape == "ladder" else _loosen_boxes(nodes, 5)
        assert not rq.same_bytes(mh.Statement(oracle, tight, tris).answer_k(mh.groups(rays, 2), 2), mh.Statement(oracle, nodes, tris).answer_k(mh.groups(rays, 2), 2))
    st = mh.Statement(oracle, nodes, tris)
    ctx = context(native, native.TRAVERSAL_BVH, (tris, mats, nodes), lab=True)
    try:
        state = ctx.scene_state(pieces=[])
        assert state["n_wide"] > 0
        if shape == "mirrored":
            assert state["wide_stack_levels"] > lds_levels, state["wide_stack_levels"]
        for k in (2, 8):
            records = mh.groups(rays, k)
            want = st.answer_k(records, k)
            assert (want.reshape(-1, k)["prim"][:, 1] != mh.NO_PRIM).sum() > 20  # rays that meet more than one triangle
            ask(ctx, records, k, f"{shape} k={k}")(want)
    finally:
        ctx.close()


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_prim_is_the_callers_index_after_a_build_form(native, oracle, default_scene, method):
    from rvpt_amd import scene
    tris, mats, _ = default_scene
    tris = tris[np.random.RandomState(2).permutation(tris.shape[0])]
    nodes, perm = {"lbvh": scene.build_lbvh, "ploc": scene.build_ploc, "sah": scene.build_sah}[method](tris)[:2]
    records = mh.groups(rq.base_rays(tris, 17, counts=(80, 160, 40, 60, 60, 21)), 4)
    want = mh.Statement(oracle, nodes, tris[perm]).answer_k(records, 4, 0, perm=perm)
    assert (want.reshape(-1, 4)["prim"][:, 3] != mh.NO_PRIM).sum() > 20
    ctx = context(native, native.TRAVERSAL_BVH, None, upload=lambda c: c.build_scene(tris, mats, method) == method or pytest.fail("fell back"))
    try:
        ask(ctx, records, 4, method)(want)
    finally:
        ctx.close()


def test_after_a_skin_update_and_a_guarded_pose_that_rebuilds(native, oracle):
    """k = 4 against the statement over the model's tree (tests/_scene_model.py): after bind + skin (a refit), then after a guarded pose update past its
    limit (a rebuild: new tree, new permutation)"""
    import _guarded_pose as gp
    import _scene_model as sm
    import _skin
    tris, mats = sm.scene_of("default143")
    limit = 1.05  # (the part turned by 90 degrees costs the tree 1.067 of its base: past this limit, not past _guarded_pose.LIMIT)
    model = sm.Model()
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, "sah") == "sah"
        model.build("sah", tris)
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
                assert report.rebuilt and report.cost > 1.06 * report.base
                assert ctx.pose_parts(moves, rebuild_above=limit).rebuilt
            records = mh.groups(rq.base_rays(model.current, 19, counts=(80, 160, 40, 60, 60, 21)), 4)
            want = mh.Statement(oracle, model.nodes, model.stored()).answer_k(records, 4, 0, perm=model.perm)
            assert (want.reshape(-1, 4)["prim"][:, 3] != mh.NO_PRIM).sum() > 15
            ask(ctx, records, 4, f"after {step}")(want)
            seen.append(model.current.tobytes())
        assert seen[0] != seen[1]
    finally:
        ctx.close()


def test_brute_force_tiles_wrap(native, oracle):
    """2 * 512 + 37 triangles are two LDS tiles and a tail; k = 8 keeps hits from every tile in one list"""
    from rvpt_amd import scene
    tile = kernel_constant("kQueryTileTris")
    assert tile == 512
    tris, mats = scene.heightfield_scene(cells=24)
    tris = np.ascontiguousarray(tris[:2 * tile + 37])
    records = mh.groups(rq.base_rays(tris, 13, counts=(40, 120, 40, 40, 40, 20)), 8)
    want = mh.Statement(oracle, None, tris).answer_k(records, 8, 1)
    prim = want.reshape(-1, 8)["prim"].astype(np.int64)
    held = prim != mh.NO_PRIM
    tiles = [(np.where(held, prim // tile, -1) == i).any(axis=1) for i in range(3)]
    assert (tiles[0] & tiles[1]).any() and (tiles[1] & tiles[2]).any()  # one list holds hits of two tiles
    ctx = context(native, native.TRAVERSAL_BRUTE, (tris, mats, None))
    try:
        ask(ctx, records, 8, "brute force, three tiles")(want)
    finally:
        ctx.close()


@pytest.mark.parametrize("flags,traversal", [KINDS[0], KINDS[3]])
def test_group_counts(native, default_scene, sweep, flags, traversal):
    """1, 63, 64, 65 and 129 groups at k = 3: the run boundaries of the claim, a last wave that is partly live — and nothing past the last group is written"""
    records, want = sweep["default", traversal, 3]
    ctx = context(native, flags_of(native, flags), default_scene)
    try:
        for n in (1, 63, 64, 65, 129):
            buf = np.concatenate([records[:3 * n], mh.groups(records[:2], 3)])  # a tail the call is not given
            got = ctx.trace_rays_into(buf[:3 * n], hits=3)
            mh.check_groups(got, want[:3 * n], records[:3 * n], f"{flags} n={n}")
            assert (buf[3 * n:].view(np.uint32).reshape(-1, 12)[:, 8:] == mh.POISON).all()
    finally:
        ctx.close()


def test_device_records_and_the_errors(native, default_scene, sweep):
    import torch
    records, want = sweep["default", 0, 3]
    n = records.shape[0] // 3
    tris, mats, nodes = default_scene
    read = lambda c, fmt, buf, nbytes: c._L.rvpt_hip_read(c._h, fmt, buf.ctypes.data_as(ctypes.c_void_p), nbytes)
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        host12 = torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12))
        with pytest.raises(native.NativeError, match="no scene to ask") as e:  # before any scene
            ctx.trace_rays_into(host12.clone(), hits=3)
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        # host array [n, k], host tensor, device tensor: the same bytes
        mh.check_groups(ctx.trace_rays_into(records.copy().reshape(n, 3), hits=3), want, records, "host [n, k]")
        host_t = host12.clone()
        assert ctx.trace_rays_into(host_t, hits=3) is host_t
        mh.check_groups(host_t.numpy().view(native.RAY_HIT_DTYPE).reshape(-1), want, records, "host tensor")
        dev = host12.to("cuda:0")
        assert ctx.trace_rays_into(dev, hits=3) is dev
        mh.check_groups(dev.cpu().numpy().view(native.RAY_HIT_DTYPE).reshape(-1), want, records, "device records")
        # a device view that starts 4 bytes in: refused, memory untouched
        flat = host12.to("cuda:0").reshape(-1)
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="16-byte alignment") as e:
            ctx.trace_rays_into(flat[1:1 + 12 * 6].reshape(6, 12), hits=3)
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        # 48 k n + 48 bytes: refused, untouched, the message names k
        buf = records[:3 * 2 + 1].copy()
        assert read(ctx, native.FORMAT_RAY_HITS_NEAREST(3), buf, 48 * 3 * 2 + 48) == native.ERR_INVALID
        said = ctx._L.rvpt_hip_last_error(ctx._h)
        assert b"k = 3" in said and b"336" in said and b"multiple" in said and buf.tobytes() == records[:7].tobytes()
        assert read(ctx, native.FORMAT_RAY_HITS_NEAREST(1), buf, 49) == native.ERR_INVALID  # k = 1 is format 2, in its message too
        said = ctx._L.rvpt_hip_last_error(ctx._h)
        assert read(ctx, native.FORMAT_RAY_HITS, buf, 49) == native.ERR_INVALID and ctx._L.rvpt_hip_last_error(ctx._h) == said and b"k =" not in said
        assert buf.tobytes() == records[:7].tobytes()
        assert read(ctx, native.FORMAT_RAY_HITS_NEAREST(3), buf, 0) == 0  # a no-op
        assert ctx.trace_rays_into(records[:0].copy(), hits=3).shape == (0,) and buf.tobytes() == records[:7].tobytes()
        for fmt in (32, 41):  # unknown, dst untouched
            assert read(ctx, fmt, buf, 48 * 6) == native.ERR_INVALID and b"unknown format %d" % fmt in ctx._L.rvpt_hip_last_error(ctx._h)
            assert buf.tobytes() == records[:7].tobytes()
        ctx.trace_rays_into(records[:3].copy(), hits=3)  # a successful query leaves last_error as it was
        assert b"unknown format 41" in ctx._L.rvpt_hip_last_error(ctx._h)
        # trace_rays builds the groups itself and repeats the ray in every record
        g = records.reshape(n, 3)
        j = int(np.flatnonzero(want.reshape(n, 3)["prim"][:, 2] != mh.NO_PRIM)[0])
        out = ctx.trace_rays(g["org"][j, 0], g["dir"][j, 0], g["tmax"][j, 0], bool(g["flags"][j, 0] & 1), hits=3)
        assert out.shape == (1, 3) and out["prim"].tolist() == want.reshape(n, 3)["prim"][j:j + 1].tolist() and (bits(out["t"]) == bits(want.reshape(n, 3)["t"][j:j + 1])).all()
        assert (out["org"] == g["org"][j, 0]).all() and (out["dir"] == g["dir"][j, 0]).all()
        # the empty scene: all k n miss quads carrying record 0's tmax bits, a NaN payload included
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        asked = records.copy().reshape(n, 3)
        asked["tmax"][::5, 0] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
        empty = ctx.trace_rays_into(asked.copy(), hits=3)
        assert (empty["prim"] == mh.NO_PRIM).all() and (bits(empty["t"]) == bits(asked["tmax"][:, :1])).all() and not empty["u"].any() and not empty["v"].any()
        assert (bits(empty["t"][::5]) == 0x7FC12345).all()
        for name in ("org", "tmax", "dir", "flags"):
            assert empty[name].tobytes() == asked[name].tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_a_query_leaves_frames_untouched(native, default_scene, sweep, flags):
    """Two accumulated frames, a k = 8 query, a third frame: image, stats, the timing's dispatch count, launch_info, cull_info and last_error equal a
    context that never asked"""
    from rvpt_amd import RenderSettings
    records, _ = sweep["default", 0, 8]
    tris, mats, nodes = default_scene
    fl = getattr(native, flags) | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for asks in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
            if asks:
                ctx.trace_rays_into(records.copy(), hits=8)  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.trace_rays_into(records.copy(), hits=8)  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info(), bytes(ctx._L.rvpt_hip_last_error(ctx._h))))
        finally:
            ctx.close()
    assert out[0] == out[1]


def _renderer(tris, traversal="bvh"):
    from rvpt_amd import RVPT, scene
    r = RVPT(64, 36, device=0, traversal=traversal)
    r.add_triangles(tris)
    for m in scene.default_materials():
        r.add_material(m)
    r.initialize()
    return r


def test_pick_lists_the_four_front_layers(native, oracle):
    """RVPT.pick(x, y, hits=4) on the layered scene: the four front layers in order, prim in the order the triangles were added — the statement's list for
    oracle.camera_ray's pixel-centre ray (pick makes its ray in double on the host: prim exactly, t to 1e-5 relative)"""
    W, H = 64, 36
    tris, zs = mh.layered_scene()
    front = sorted(zs[::2])[:4]
    r = _renderer(tris)
    try:
        cam = r.scene_camera.get_data()
        st = mh.Statement(oracle, r.bvh_nodes, r.sorted_triangles)
        order = np.asarray(r.primitive_indices)
        for x, y in ((32, 18), (30, 20)):
            o, d = oracle.camera_ray(0, cam, (x + 0.5) / W, 1.0 - (y + 0.5) / H)
            want = st.trace_k(o, d, 4)
            got = r.pick(x, y, hits=4)
            assert len(got) == len(want) == 4 and [p for p, _ in got] == [int(order[h[0]]) for h in want]
            assert all(abs(t - float(h[1])) <= 1e-5 * float(h[1]) for (_, t), h in zip(got, want))
            assert [zs[p] for p, _ in got] == front and [t for _, t in got] == sorted(t for _, t in got)
            assert r.pick(x, y) == got[0]
            assert len(r.pick(x, y, hits=8)) == 8
        o, d = oracle.camera_ray(0, cam, 0.5 / W, 1.0 - 0.5 / H)  # the corner pixel's ray passes beside the quads: a miss is the empty list
        assert st.trace_k(o, d, 4) == [] and r.pick(0, 0, hits=4) == [] and r.pick(0, 0) is None
    finally:
        r.shutdown()


def test_rvpt_trace_rays_numbers_prim_in_the_order_added(native, oracle):
    """RVPT.trace_rays(hits=2) on a host-built tree: prim of both slots numbers the triangles as they were added"""
    tris, zs = mh.layered_scene()
    rays = mh.through_rays(40, 37)
    r = _renderer(tris)
    try:
        got = r.trace_rays(rays["org"], rays["dir"], hits=2)
        want = mh.Statement(oracle, r.bvh_nodes, r.sorted_triangles).answer_k(mh.groups(rays, 2), 2, 0, perm=np.asarray(r.primitive_indices)).reshape(-1, 2)
        assert got.shape == (40, 2) and got["prim"].tolist() == want["prim"].tolist() and got["t"].tobytes() == want["t"].tobytes()
        assert (zs[got["prim"][:, 0]] == 1.0).all() and (zs[got["prim"][:, 1]] == 1.5).all()
        assert not (np.asarray(r.primitive_indices) == np.arange(tris.shape[0])).all()  # the leaf order is not the order added
    finally:
        r.shutdown()
