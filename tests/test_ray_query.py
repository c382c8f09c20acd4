"""Ray queries on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_RAY_HITS (Context.trace_rays / trace_rays_into) against the statement of tests/_ray_query.py — the
reference's walk over the oracle's box and triangle tests.  Everything is bit-exact: the kernels are deterministic per ray, so whole records are compared
byte for byte, no tolerance and no ray left out (the one exception, RVPT.pick, makes its ray on the host and says so)."""
import re
from pathlib import Path

import numpy as np
import pytest

import _ray_query as rq
from _util import identity_camera
from test_gpu_parity import _chain_bvh, _loosen_boxes
from test_refit import bits, extent

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def kernel_constant(name):
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", (ROOT / "rvpt_amd" / "csrc" / "rvpt_query.h").read_text()).group(1))


@pytest.fixture(scope="module")
def ray_set(oracle, default_scene):
    """(records, the statement's answer on the tree, ... in stored order): 2048 + 37 rays of every kind, a third any-hit; for each that hits the six tmax
    variants; a dozen non-finite records.  Computed once, never changed: every case that asks the default scene shares it."""
    tris, _, nodes = default_scene
    st = rq.Statement(oracle, nodes, tris)
    base = rq.base_rays(tris, 7)
    assert base.shape[0] == 2048 + 37
    records = rq.poisoned(np.concatenate([rq.with_tmax_variants(base, st.answer(base)), rq.non_finite_records(base, 9, 12)]))
    assert records.shape[0] % 64 and records.shape[0] % 256
    want = {0: st.answer(records, 0), 1: st.answer(records, 1)}
    for w in want.values():
        w.setflags(write=False)
    records.setflags(write=False)
    hits = int((want[0]["prim"] != rq.NO_PRIM).sum())
    assert 500 < hits < records.shape[0] - 500, hits
    assert (want[0]["prim"][-12:] == rq.NO_PRIM).all()
    assert not rq.same_bytes(want[0], want[1])  # the two orders do differ somewhere (ties, any hit): the cases below tell them apart
    return records, want


def ask(native, flags, scene3, records, lab=None, upload=None):
    ctx = native.Context(64, 36, 0, 0, 1, flags, lab=lab)
    try:
        if upload is not None:
            upload(ctx)
        else:
            tris, mats, nodes = scene3
            ctx.upload_scene(nodes if flags & 3 else None, tris, mats)
        got = ctx.trace_rays_into(records.copy())
        state = ctx.scene_state(pieces=[]) if lab else None
        return got, state
    finally:
        ctx.close()


def check(got, want, records, what):
    assert rq.same_bytes(got, want), f"{what}: {rq.first_difference(got, want)}"
    for name in ("org", "tmax", "dir", "flags"):  # the in fields come back byte for byte, NaN payloads included
        assert got[name].tobytes() == records[name].tobytes(), (what, name)


@pytest.mark.parametrize("flags,traversal", [("TRAVERSAL_BVH", 0), ("TRAVERSAL_BVH_ORDERED", 0), ("TRAVERSAL_BVH|BVH_PER_LANE", 0), ("TRAVERSAL_BRUTE", 1)])
def test_queries_answer_as_the_statement(native, default_scene, ray_set, flags, traversal):
    """Case 1.  BVH contexts of every flavour — the ordered one too: a query never walks nearer-child-first — give traversal 0's answers over the wide form
    (which the laboratory build's read-back shows to exist), brute-force contexts traversal 1's; the non-finite records are misses."""
    records, want = ray_set
    fl = 0
    for name in flags.split("|"):
        fl |= getattr(native, name)
    got, _ = ask(native, fl, default_scene, records)
    check(got, want[traversal], records, flags)
    assert (got["prim"][-12:] == rq.NO_PRIM).all() and got["t"][-12:].tobytes() == records["tmax"][-12:].tobytes()
    if traversal == 0:
        lab_got, state = ask(native, fl, default_scene, records, lab=True)
        assert state["n_wide"] > 0 and state["bvh_head_shift"] > 0
        check(lab_got, want[0], records, flags + " (laboratory build)")


def _mirrored_chain(tris):
    """_chain_bvh with the children of every inner node swapped: the REST of the chain on the left, the leaf on the right — the walk goes down the chain
    first and every level leaves a leaf on the stack.  Inner node k sits at 0, 1, 3, 5, ..., its children at 2k + 1 (the rest) and 2k + 2 (leaf k)."""
    chain = _chain_bvh(tris)  # inner node k at 2k, leaf k at 2k + 1, the last leaf at 2n - 2
    n = tris.shape[0]
    out = chain.copy()
    at = 0
    for k in range(n - 1):
        out[at] = (2 * k + 1, 0, chain[2 * k]["bounds"])
        out[2 * k + 2] = chain[2 * k + 1]
        at = 2 * k + 1
    out[at] = chain[2 * n - 2]
    return out


@pytest.mark.parametrize("loose", [False, True])
@pytest.mark.parametrize("shape", ["chain", "mirrored"])
def test_the_overflow_stack(native, oracle, shape, loose):
    """Case 2.  Stacks deeper than the kQueryLdsLevels = 8 slots a lane keeps in LDS (rvpt_query.h), on 48 triangles.  _chain_bvh puts every leaf on the LEFT:
    its wide form never holds more than 3 slots at once (wide_stack_levels = 3, from rvpt_bvh_wide_form), so it stays inside LDS — kept as the shape the
    frame tests use.  The mirrored chain puts the leaves on the right: wide_stack_levels = 47 > 8 (asserted below from the read-back), and the walk really goes
    through the global columns.  A few hundred rays each, on the tight tree and on a loosened one; the binary walk's turn is test_binary_walk_past_the_lds_levels."""
    from rvpt_amd import scene
    lds_levels = kernel_constant("kQueryLdsLevels")
    assert lds_levels == 8
    rng = np.random.RandomState(11)
    quads = []
    for k in range(24):
        z, s, c = 1.0 + 0.25 * k, 0.3 + 0.05 * k, rng.uniform(-0.5, 0.5, 2)
        p = [(c[0] - s, c[1] - s, z), (c[0] + s, c[1] - s, z), (c[0] + s, c[1] + s, z), (c[0] - s, c[1] + s, z)]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    tris = scene.make_triangles(quads, 0)
    mats = scene.default_materials()
    nodes = _chain_bvh(tris) if shape == "chain" else _mirrored_chain(tris)
    if loose:
        nodes = _loosen_boxes(nodes, 5)
    records = rq.base_rays(tris, 3, counts=(60, 100, 40, 40, 40, 20))
    st = rq.Statement(oracle, nodes, tris)
    want = st.answer(records)
    assert (want["prim"] != rq.NO_PRIM).sum() > 60
    if shape == "chain":
        assert not loose or not rq.same_bytes(want, rq.Statement(oracle, _chain_bvh(tris), tris).answer(records))  # the loosened boxes do cull
    got, state = ask(native, native.TRAVERSAL_BVH, (tris, mats, nodes), records, lab=True)
    assert state["n_wide"] > 0
    if shape == "mirrored":
        assert state["wide_stack_levels"] > lds_levels, state["wide_stack_levels"]
    check(got, want, records, f"{shape} wide")
    got, _ = ask(native, native.TRAVERSAL_BVH, (tris, mats, nodes), records)
    check(got, want, records, f"{shape} wide, release build")


def test_no_wide_form(native, default_scene, ray_set, monkeypatch):
    """Case 3.  The laboratory build with the caller-layout knob holds no wide form: walk_bvh2<Closest> gives case 1's bytes."""
    records, want = ray_set
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    got, state = ask(native, native.TRAVERSAL_BVH, default_scene, records, lab=True)
    assert state["n_wide"] == 0 and state["bvh_height"] > 0
    check(got, want[0], records, "binary walk")


def test_binary_walk_past_the_lds_levels(native, oracle, monkeypatch):
    """Case 3, deeper: 48-level chains, whose binary stack is sized past the 8 LDS levels — the mirrored one fills it (a leaf stacked per level)."""
    from rvpt_amd import scene
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    tris, mats = scene.default_scene()
    tris = tris[:48]
    for nodes in (_chain_bvh(tris), _mirrored_chain(tris)):
        records = rq.base_rays(tris, 5, counts=(60, 100, 40, 40, 40, 20))
        want = rq.Statement(oracle, nodes, tris).answer(records)
        got, state = ask(native, native.TRAVERSAL_BVH, (tris, mats, nodes), records, lab=True)
        assert state["n_wide"] == 0 and state["bvh_height"] == 48 > kernel_constant("kQueryLdsLevels")
        check(got, want, records, "binary walk, chain")


def test_brute_force_tiles_wrap(native, oracle):
    """Case 4.  kQueryTileTris = 512 triangles per LDS tile: 2 * 512 + 37 = 1061 triangles (above the 1024 a frame kernel keeps resident) are two tiles and a
    tail.  A few hundred rays against traversal 1."""
    from rvpt_amd import scene
    tile = kernel_constant("kQueryTileTris")
    assert tile == 512
    tris, mats = scene.heightfield_scene(cells=24)  # 1152 triangles
    tris = np.ascontiguousarray(tris[:2 * tile + 37])
    records = rq.base_rays(tris, 13, counts=(40, 120, 40, 40, 40, 20))
    want = rq.Statement(oracle, None, tris).answer(records, 1)
    hit = want["prim"][want["prim"] != rq.NO_PRIM]
    assert (hit < tile).any() and ((hit >= tile) & (hit < 2 * tile)).any() and (hit >= 2 * tile).any()  # every tile answers somebody
    got, _ = ask(native, native.TRAVERSAL_BRUTE, (tris, mats, None), records)
    check(got, want, records, "brute force, three tiles")


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_prim_is_the_callers_index_after_a_build_form(native, oracle, default_scene, method):
    """Case 5.  build_scene on shuffled triangles: prim numbers the CALLER'S order.  The statement runs on the numpy tree over tris[perm]; its answer goes
    through perm."""
    from rvpt_amd import scene
    tris, mats, _ = default_scene
    tris = tris[np.random.RandomState(2).permutation(tris.shape[0])]
    nodes, perm = {"lbvh": scene.build_lbvh, "ploc": scene.build_ploc, "sah": scene.build_sah}[method](tris)[:2]
    records = rq.base_rays(tris, 17, counts=(80, 160, 40, 60, 60, 21))
    want = rq.Statement(oracle, nodes, tris[perm]).answer(records, 0, perm=perm)
    assert (want["prim"] != rq.NO_PRIM).sum() > 100
    got, _ = ask(native, native.TRAVERSAL_BVH, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, method) == method or pytest.fail("fell back"))
    check(got, want, records, method)
    v = tris.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    for r in got[got["prim"] != rq.NO_PRIM][:50]:  # and it IS that triangle of the caller's array: the hit point lies in its plane
        a, b, c = v[r["prim"]]
        p = r["org"].astype(np.float64) + float(r["t"]) * r["dir"].astype(np.float64)
        n = np.cross(b - a, c - a)
        assert abs(np.dot(p - a, n)) <= 1e-4 * np.linalg.norm(n) * (1 + np.linalg.norm(p))


def test_a_walk_down_a_device_built_tree_of_37_levels(native, oracle):
    """Case 5, deep.  tests/_device_state.py's geometric ladder built by "sah": thirty levels that peel one triangle each, then the cluster in median splits
    (rv::kSahBalanceDepth) — leaves 36 levels below the root.  One ray at every triangle, from 4 h above its centroid straight down, tmax = 8 h, a third any
    hit; 64 more displaced by 3 h in z, past every triangle.  On the ladder of the generator's defaults (top 2^75, h 2^-60) no ray at all can hit the cluster: the
    triangle test's determinant is 2^-240, zero in float32 (ds.HITTABLE_LADDER says it in full), so this is that ladder with 17 between the rungs and
    h = 2^-32; the rays are the ones described.  What the rays must be is asserted of the statement before the GPU is asked."""
    import _device_state as ds
    from rvpt_amd import scene
    h = ds.HITTABLE_LADDER["h"]
    tris = ds.ladder(**ds.HITTABLE_LADDER)
    mats = scene.default_materials()
    n = tris.shape[0]
    nodes, perm, info = scene.build_sah(tris)
    assert info == {k: v for k, v in ds.LADDERS[(30, 300, 1)].items() if k != "n"}
    centroid = ds.vertices(tris).astype(np.float64).mean(axis=1)
    org = np.concatenate([centroid + [0.0, 4.0 * h, 0.0], centroid[:64] + [0.0, 4.0 * h, 3.0 * h]])
    flags = np.where(np.arange(n + 64) % 3 == 0, native.RAY_ANY_HIT, 0).astype(np.uint32)
    records = rq.make_records(org, np.tile([0.0, -1.0, 0.0], (n + 64, 1)), np.float32(8.0 * h), flags)
    want = rq.Statement(oracle, nodes, tris[perm]).answer(records, 0, perm=perm)
    hit = want["prim"][:n] != rq.NO_PRIM
    assert 4 * int(hit.sum()) >= 3 * n, int(hit.sum())
    assert (want["prim"][n:] == rq.NO_PRIM).all()
    depth_of = np.zeros(len(nodes), dtype=np.int64)  # a numpy builder's tree is breadth first: parents come before their children
    leaf_at = np.zeros(n, dtype=np.int64)  # the depth of the leaf that holds a stored position
    for i in range(len(nodes)):
        f, c = int(nodes[i]["first"]), int(nodes[i]["count"])
        if c == 0:
            depth_of[f] = depth_of[f + 1] = depth_of[i] + 1
        else:
            leaf_at[f:f + c] = depth_of[i]
    deepest = leaf_at[np.argsort(perm)[want["prim"][:n][hit]]]
    assert (deepest >= 31).any() and deepest.max() == 36
    assert (want["prim"][:n][hit] != np.flatnonzero(hit)).any()  # the cluster's triangles overlap: some rays meet a nearer one than their own
    got, state = ask(native, native.TRAVERSAL_BVH, None, records, lab=True, upload=lambda ctx: ctx.build_scene(tris, mats, "sah") == "sah" or pytest.fail("fell back"))
    assert state["bvh_height"] == 37 and state["n_wide"] > 0
    check(got, want, records, "ladder, sah")
    got, _ = ask(native, native.TRAVERSAL_BVH, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, "sah") == "sah" or pytest.fail("fell back"))
    check(got, want, records, "ladder, sah, release build")


@pytest.mark.parametrize("form", ["plain", "sparse"])
def test_queries_answer_for_the_moved_mesh(native, oracle, default_scene, form):
    """Case 6.  After update_triangles — plain, and indices= on a loose tree — a query answers for the moved mesh: the statement runs on refit_bvh(...)
    (touched= for the sparse form, which leaves the boxes off the touched paths loose)."""
    from rvpt_amd import scene
    tris, mats, nodes = default_scene
    moved = scene.wobble(tris, 1.9, 0.1 * extent(tris))
    records = rq.base_rays(tris, 19, counts=(80, 160, 40, 60, 60, 21))
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        if form == "plain":
            ctx.upload_scene(nodes, tris, mats)
            before = ctx.trace_rays_into(records.copy())
            ctx.update_triangles(moved)
            patched, refit = moved, scene.refit_bvh(nodes, moved)
        else:
            loose = _loosen_boxes(nodes, 5)
            ctx.upload_scene(loose, tris, mats)
            before = ctx.trace_rays_into(records.copy())
            idx = np.random.RandomState(7).permutation(tris.shape[0])[:tris.shape[0] // 3]
            patched = tris.copy()
            patched[idx, :12] = moved[idx, :12]
            ctx.update_triangles(patched[idx], indices=idx)
            refit = scene.refit_bvh(loose, patched, touched=idx)
        got = ctx.trace_rays_into(records.copy())
    finally:
        ctx.close()
    want = rq.Statement(oracle, refit, patched).answer(records)
    check(got, want, records, form)
    assert not rq.same_bytes(got, before)


def test_device_records_and_the_errors(native, default_scene, ray_set):
    """Case 7.  A torch tensor on cuda:0, in place: the bytes a host query returns.  A view 4 bytes in, 47 and 49 bytes, no scene: INVALID, memory untouched.
    n = 0 and n = 1.  The empty scene: all misses."""
    import ctypes
    import torch
    records, want = ray_set
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        host12 = torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12))
        with pytest.raises(native.NativeError, match="no scene to ask") as e:
            ctx.trace_rays_into(host12.clone())
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        dev = host12.to("cuda:0")
        assert ctx.trace_rays_into(dev) is dev
        got = dev.cpu().numpy().view(native.RAY_HIT_DTYPE).reshape(-1)
        check(got, want[0], records, "device records")
        host_t = host12.clone()  # a host tensor goes the host way
        ctx.trace_rays_into(host_t)
        check(host_t.numpy().view(native.RAY_HIT_DTYPE).reshape(-1), want[0], records, "host tensor")
        # a view that starts 4 bytes in: device records need 16-byte alignment
        flat = host12.to("cuda:0").reshape(-1)
        keep = flat.clone()
        view = flat[1:1 + 12 * 5].reshape(5, 12)
        with pytest.raises(native.NativeError, match="16-byte alignment") as e:
            ctx.trace_rays_into(view)
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        # byte counts that are no whole number of records, through the C call
        buf = records[:2].copy()
        for nbytes in (47, 49):
            rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_RAY_HITS, buf.ctypes.data_as(ctypes.c_void_p), nbytes)
            assert rc == native.ERR_INVALID and b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h)
            assert buf.tobytes() == records[:2].tobytes()
        # a successful query leaves last_error as it was
        ctx.trace_rays_into(records[:1].copy())
        assert b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h)
        # n = 0 and n = 1
        assert ctx.trace_rays_into(records[:0].copy()).shape == (0,)
        assert ctx.trace_rays_into(torch.zeros((0, 12), device="cuda:0")).shape == (0, 12)
        k = int(np.flatnonzero(want[0]["prim"] != rq.NO_PRIM)[0])
        check(ctx.trace_rays_into(records[k:k + 1].copy()), want[0][k:k + 1], records[k:k + 1], "one record")
        one = torch.from_numpy(records[k:k + 1].copy().view(np.float32).reshape(1, 12)).to("cuda:0")
        check(ctx.trace_rays_into(one).cpu().numpy().view(native.RAY_HIT_DTYPE).reshape(-1), want[0][k:k + 1], records[k:k + 1], "one device record")
        # trace_rays builds the records itself
        r = records[k]
        out = ctx.trace_rays(r["org"], r["dir"], r["tmax"], bool(r["flags"] & native.RAY_ANY_HIT))
        assert out.dtype == native.RAY_HIT_DTYPE and out[0]["prim"] == want[0]["prim"][k] and bits(out["t"])[0] == bits(want[0]["t"])[k]
        # the empty scene answers every ray with a miss
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        empty = ctx.trace_rays_into(records.copy())
        assert (empty["prim"] == rq.NO_PRIM).all() and empty["t"].tobytes() == records["tmax"].tobytes() and not empty["u"].any() and not empty["v"].any()
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_a_query_leaves_frames_untouched(native, default_scene, ray_set, flags):
    """Case 8.  Two accumulated frames, a query, a third frame: image, stats, the timing's dispatch count, launch_info and cull_info equal a context that
    never asked."""
    from rvpt_amd import RenderSettings
    records, _ = ray_set
    tris, mats, nodes = default_scene
    fl = getattr(native, flags) | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for asks in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
            if asks:
                ctx.trace_rays_into(records[:300].copy())  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.trace_rays_into(records.copy())  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info()))
        finally:
            ctx.close()
    assert out[0] == out[1]


def test_any_rank_of_a_partition_answers(native, default_scene, ray_set):
    """Case 9.  tile_world = 2 without a communicator: rank 1's context holds the whole scene and returns case 1's bytes."""
    records, want = ray_set
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 1, 2, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, tris, mats)
        check(ctx.trace_rays_into(records.copy()), want[0], records, "rank 1 of 2")
    finally:
        ctx.close()


def test_pick_is_the_pixel_centre_ray(native, oracle):
    """Case 10.  RVPT.pick at three pixels of a 64 x 36 frame names the triangle the statement names for oracle.camera_ray's pixel-centre ray.  pick makes its
    direction in double on the HOST (the one place the host makes a ray), the oracle in float32 as a frame does: prim is compared exactly, t to 1e-5 relative."""
    from rvpt_amd import RVPT, scene
    W, H = 64, 36
    tris, mats = scene.default_scene()
    r = RVPT(W, H, device=0, traversal="bvh")
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        r.scene_camera.translation = np.array([0.0, 0.8, -1.5])  # the model fills the middle of the frame
        cam = r.scene_camera.get_data()
        st = rq.Statement(oracle, r.bvh_nodes, r.sorted_triangles)
        order = np.asarray(r.primitive_indices)
        seen = 0
        for x, y in ((32, 18), (36, 22), (2, 1)):
            o, d = oracle.camera_ray(0, cam, (x + 0.5) / W, 1.0 - (y + 0.5) / H)
            prim, t, _, _ = st.trace(o, d)
            got = r.pick(x, y)
            if prim == rq.NO_PRIM:
                assert got is None
            else:
                seen += 1
                assert got is not None and got[0] == order[prim] and abs(got[1] - float(t)) <= 1e-5 * float(t)
        assert seen >= 2
        r.scene_camera.mode = 1
        with pytest.raises(ValueError, match="pinhole"):
            r.pick(1, 1)
    finally:
        r.shutdown()
