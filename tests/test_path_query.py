"""Path queries on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_RAY_PATHS (Context.trace_paths / trace_paths_into) against oracle.render.  The records are the
ones a frame's pixels would ask with (tests/_path_query.py); `0 + radiance`, scaled as a first frame scales it, must be the rendered image bit for bit at every
pixel, and the segments must add up to the render's count.  Everything is bit-exact: a record's answer is a function of its 32 in bytes and the scene, so out
fields are compared byte for byte — across host and device records, across contexts, and across every way of batching and ordering the records."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _path_query as pq
from _util import identity_camera, scene_by_name
from test_ray_query import _mirrored_chain

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
W, H = 48, 32
IN = ("org", "seed", "dir", "max_bounces")


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def kernel_constant(name, header="rvpt_paths.h"):
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", (ROOT / "rvpt_amd" / "csrc" / header).read_text()).group(1))


def camera_at(translation):
    from rvpt_amd.camera import Camera
    camera = Camera(W / H)
    camera.translation = np.array(translation, dtype=np.float64)
    return camera.get_data()


_records = {}


def records_for(oracle, cam, mode, frame, budget):
    """the frame's records, derived once per (camera, mode, frame) and never changed; the budget is set on a copy"""
    key = (cam.tobytes(), mode, frame)
    if key not in _records:
        rec = pq.frame_records(oracle, mode, cam, W, H, frame, 0)
        rec.setflags(write=False)
        _records[key] = rec
    rec = _records[key].copy()
    rec["max_bounces"] = budget
    return rec


def on_device(records):
    import torch
    return torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12)).to("cuda:0")


def from_device(native, tensor):
    return tensor.cpu().numpy().view(native.RAY_PATH_DTYPE).reshape(-1)


def out_bytes(rec):
    return rec["radiance"].tobytes() + rec["segments"].tobytes()


def check_ins(got, records, what):
    for name in IN:  # the in fields come back byte for byte
        assert got[name].tobytes() == records[name].tobytes(), (what, name)


def check_against_render(oracle, native, ctx, rec, cam, scene3, traversal, mode, frame, budget, what):
    """host records and device records: the oracle's image and segment count, and each other's bytes"""
    tris, mats, nodes = scene3
    settings = oracle.settings_bytes(max_bounces=budget, aa=1, current_frame=frame, camera_mode=mode)
    img, stats = oracle.render(settings, cam, nodes if traversal == 0 else None, tris, mats, W, H, traversal)
    host = ctx.trace_paths_into(rec.copy())
    dev = from_device(native, ctx.trace_paths_into(on_device(rec)))
    for got, where in ((host, "host records"), (dev, "device records")):
        check_ins(got, rec, f"{what}, {where}")
        image = pq.expected_image(got["radiance"], frame, W, H)
        print(f"{what}, {where}: {int((pq.bits(image) != pq.bits(img[..., :3])).any(axis=-1).sum())} of {W * H} pixels differ, "
              f"segments {int(got['segments'].sum(dtype=np.uint64))} against {int(stats[0])}")
        assert pq.same_bits(image, img[..., :3]), f"{what}, {where}: {pq.first_difference(image, img[..., :3])}"
        assert int(got["segments"].sum(dtype=np.uint64)) == int(stats[0]), (what, where)
        assert (got["segments"] >= 1).all() and (got["segments"] <= budget).all()
    assert out_bytes(host) == out_bytes(dev), what
    return host


def make_context(native, kind, scene3, extra_flags=0, lab=None):
    flags = {"brute": native.TRAVERSAL_BRUTE, "bvh": native.TRAVERSAL_BVH, "ordered": native.TRAVERSAL_BVH_ORDERED}[kind] | extra_flags
    ctx = native.Context(W, H, 0, 0, 1, flags, lab=lab)
    tris, mats, nodes = scene3
    ctx.upload_scene(nodes if kind != "brute" else None, tris, mats)
    return ctx


@pytest.fixture(scope="module")
def showcase():
    return scene_by_name("showcase")


@pytest.fixture(scope="module")
def showcase_cam():
    return camera_at((0.0, 0.9, -2.5))


@pytest.fixture(scope="module")
def cornell():
    return scene_by_name("cornell")


@pytest.fixture(scope="module")
def cornell_cam():
    return camera_at((0.0, 2.0, -1.9))  # inside the box, looking at its back wall: every pixel hits


# ---- 1. parity with the reference integrator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_radiance_is_the_reference_integrators(native, oracle, showcase, showcase_cam, mode, kind):
    """48 x 32 on the showcase scene (mirror, glass, emitter), pinhole / orthographic / spherical camera, budgets 1, 2 and 8, frames 0 and 5"""
    ctx = make_context(native, kind, showcase)
    try:
        for frame in (0, 5):
            for budget in (1, 2, 8):
                rec = records_for(oracle, showcase_cam, mode, frame, budget)
                got = check_against_render(oracle, native, ctx, rec, showcase_cam, showcase, 1 if kind == "brute" else 0, mode, frame, budget, f"mode {mode} {kind} frame {frame} budget {budget}")
                if mode == 0 and frame == 0 and budget > 1:
                    assert int((got["segments"] > 1).sum()) == 834  # the pixels whose camera ray hits geometry go on
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["bvh", "brute"])
def test_deep_paths_inside_the_cornell_box(native, oracle, cornell, cornell_cam, kind):
    """9164 triangles from inside the box: every pixel hits, paths run to the budget of 8.  BVH: the 4-wide walk through HBM-resident nodes; brute force:
    eighteen LDS tiles, the last one partial."""
    assert cornell[0].shape[0] == 9164 and 9164 % kernel_constant("kQueryTileTris", "rvpt_query.h")
    ctx = make_context(native, kind, cornell)
    try:
        rec = records_for(oracle, cornell_cam, 0, 0, 8)
        got = check_against_render(oracle, native, ctx, rec, cornell_cam, cornell, 1 if kind == "brute" else 0, 0, 0, 8, f"cornell {kind}")
        assert (got["segments"] > 1).all() and (got["segments"] == 8).sum() > 100
    finally:
        ctx.close()


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_deep_paths_on_a_device_built_tree(native, oracle, cornell, cornell_cam, method):
    """The same on a context whose tree the device built from shuffled triangles: radiance does not depend on the numbering, the walk order depends on the tree —
    the oracle gets the numpy statement of that tree."""
    from rvpt_amd import scene
    tris, mats, _ = cornell
    tris = tris[np.random.RandomState(2).permutation(tris.shape[0])]
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        built = ctx.build_scene(tris, mats, method)  # ("ploc" may fall back to the LBVH tree by its stated rule: the statement follows what was built)
        assert built == method or (method, built) == ("ploc", "lbvh")
        nodes, perm = {"lbvh": scene.build_lbvh, "ploc": scene.build_ploc, "sah": scene.build_sah}[built](tris)[:2]
        rec = records_for(oracle, cornell_cam, 0, 0, 8)
        check_against_render(oracle, native, ctx, rec, cornell_cam, (tris[perm], mats, nodes), 0, 0, 0, 8, f"cornell built by {method}")
    finally:
        ctx.close()


# ---- 2. parity with the context's own frame -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_radiance_is_the_contexts_own_frame(native, oracle, showcase, showcase_cam, mode, kind):
    """Same records, same context: the frame read back is 0 + radiance (scaled as a first frame is), and the frame's segment count is the records' sum"""
    from rvpt_amd import RenderSettings
    ctx = make_context(native, kind, showcase, native.COUNT_SEGMENTS)
    try:
        for frame in (0, 5):
            rec = records_for(oracle, showcase_cam, mode, frame, 8)
            got = ctx.trace_paths_into(rec.copy())
            before = ctx.stats()[0]
            ctx.set_frame(RenderSettings(max_bounces=8, aa=1, current_frame=frame, camera_mode=mode).pack(), showcase_cam)
            ctx.dispatch()
            img = ctx.read()
            image = pq.expected_image(got["radiance"], frame, W, H)
            assert pq.same_bits(image, img[..., :3]), f"mode {mode} {kind} frame {frame}: {pq.first_difference(image, img[..., :3])}"
            assert ctx.stats()[0] - before == int(got["segments"].sum(dtype=np.uint64))
            ctx.write_accum(np.zeros((H, W, 4), np.float32))  # (the next frame of this loop starts from nothing, as the oracle's)
    finally:
        ctx.close()


def test_an_ordered_context_answers_as_a_plain_one(native, oracle, showcase, showcase_cam, cornell, cornell_cam):
    """A query never walks nearer-child-first: on a BVH_ORDERED context its bytes are a plain BVH context's — not necessarily the ordered frame's"""
    for scene3, cam in ((showcase, showcase_cam), (cornell, cornell_cam)):
        rec = records_for(oracle, cam, 0, 0, 8)
        out = []
        for kind in ("bvh", "ordered"):
            ctx = make_context(native, kind, scene3)
            try:
                out.append(ctx.trace_paths_into(rec.copy()))
            finally:
                ctx.close()
        assert out[0].tobytes() == out[1].tobytes()


# ---- 3. independence from position and batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
def test_a_records_answer_does_not_depend_on_its_batch(native, oracle, showcase, showcase_cam, kind):
    """What regeneration could break.  The 1536 records permuted at random, then split into calls of 1, 63, 64, 65, 257 and the rest: every record's 16 out
    bytes are the one-call answer's.  A batch that mixes budgets of 1 and 8 with invalid records answers each record as it is answered alone."""
    ctx = make_context(native, kind, showcase)
    try:
        rec = records_for(oracle, showcase_cam, 0, 0, 8)
        whole = ctx.trace_paths_into(rec.copy())
        rng = np.random.RandomState(23)
        order = rng.permutation(rec.shape[0])
        shuffled = ctx.trace_paths_into(rec[order].copy())
        assert shuffled.tobytes() == whole[order].tobytes()
        parts, at = [], 0
        for size in (1, 63, 64, 65, 257, rec.shape[0] - (1 + 63 + 64 + 65 + 257)):
            parts.append(ctx.trace_paths_into(rec[order][at:at + size].copy()))
            at += size
        assert at == rec.shape[0] and np.concatenate(parts).tobytes() == whole[order].tobytes()
        dev_parts, at = [], 0
        for size in (65, 1, rec.shape[0] - 66):  # ... and from device memory
            dev_parts.append(from_device(native, ctx.trace_paths_into(on_device(rec[order][at:at + size]))))
            at += size
        assert np.concatenate(dev_parts).tobytes() == whole[order].tobytes()
        # budgets of 1 and 8 and invalid records in one batch
        ones = rec.copy()
        ones["max_bounces"] = 1
        whole_ones = ctx.trace_paths_into(ones.copy())
        mixed = rec.copy()
        pick = rng.randint(0, 3, rec.shape[0])
        mixed["max_bounces"][pick == 1] = 1
        bad = np.flatnonzero(pick == 2)
        mixed["max_bounces"][bad[0::3]] = 0
        mixed["max_bounces"][bad[1::3]] = native.PATH_MAX_BOUNCES + 1
        mixed["dir"][bad[2::3], 1] = np.nan
        mixed = mixed[order]
        got = ctx.trace_paths_into(mixed.copy())
        check_ins(got, mixed, "mixed batch")
        want = out_view(whole).copy()
        want[pick == 1] = out_view(whole_ones)[pick == 1]
        want[pick == 2] = np.zeros(1, dtype="V16")[0]
        want = want[order]
        assert out_view(got).tobytes() == want.tobytes()
        for k in rng.permutation(rec.shape[0])[:12]:  # and really alone: a dozen one-record calls
            assert ctx.trace_paths_into(mixed[k:k + 1].copy()).tobytes() == got[k:k + 1].tobytes()
    finally:
        ctx.close()


def out_view(rec):
    """the 16 out bytes of every record as one void scalar each"""
    return np.ascontiguousarray(rec.view(np.uint8).reshape(-1, 48)[:, 32:]).view("V16").reshape(-1)


# ---- 4. deep tree ---------------------------------------------------------------------------------------------------------------------------------------
def chain_scene():
    """24 quads one behind the other along +z, growing with the distance, with materials that bounce (Lambert, mirror, glass in turn; an emitter at the far
    end), under the mirrored chain tree: every level leaves a leaf on the stack"""
    from rvpt_amd import scene
    rng = np.random.RandomState(11)
    quads, ids = [], []
    for k in range(24):
        z, s, c = 1.0 + 0.25 * k, 0.3 + 0.05 * k, rng.uniform(-0.5, 0.5, 2)
        p = [(c[0] - s, c[1] - s, z), (c[0] + s, c[1] - s, z), (c[0] + s, c[1] + s, z), (c[0] - s, c[1] + s, z)]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
        ids += [3 if k == 23 else k % 3] * 2
    tris = scene.make_triangles(quads, 0)
    tris[:, 12] = np.asarray(ids, dtype=np.float32)
    return tris, scene.materials_showcase_scene()[1], _mirrored_chain(tris)


@pytest.mark.parametrize("walk", ["wide", "binary"])
def test_paths_through_the_overflow_stack(native, oracle, monkeypatch, walk):
    """The mirrored chain's wide form holds 47 slots at once, its binary walk 48: past the kQueryLdsLevels = 8 a lane keeps in LDS, so the walks go through the
    global columns — path_bvh4, and path_bvh2 on a laboratory context that holds no wide form.  A camera at the origin looks along the chain."""
    if walk == "binary":
        monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    scene3 = chain_scene()
    cam = identity_camera(W / H)
    ctx = make_context(native, "bvh", scene3, lab=True)
    try:
        state = ctx.scene_state(pieces=[])
        lds_levels = kernel_constant("kQueryLdsLevels", "rvpt_query.h")
        if walk == "wide":
            assert state["n_wide"] > 0 and state["wide_stack_levels"] > lds_levels
        else:
            assert state["n_wide"] == 0 and state["bvh_height"] > lds_levels
        for mode in (0, 2):
            rec = records_for(oracle, cam, mode, 0, 8)
            got = check_against_render(oracle, native, ctx, rec, cam, scene3, 0, mode, 0, 8, f"chain, {walk} walk, mode {mode}")
            assert mode != 0 or (got["segments"] > 1).sum() > 50
    finally:
        ctx.close()
    if walk == "wide":  # the release build too
        ctx = make_context(native, "bvh", scene3)
        try:
            rec = records_for(oracle, cam, 0, 0, 8)
            check_against_render(oracle, native, ctx, rec, cam, scene3, 0, 0, 0, 8, "chain, release build")
        finally:
            ctx.close()


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_records_the_empty_scene_and_the_errors(native, oracle, showcase, showcase_cam):
    import torch
    tris, mats, nodes = showcase
    rec = records_for(oracle, showcase_cam, 0, 0, 8)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        # no scene yet
        untouched = rec[:3].copy()
        with pytest.raises(native.NativeError, match="path query before any full upload_scene") as e:
            ctx.trace_paths_into(untouched)
        assert e.value.code == native.ERR_INVALID and untouched.tobytes() == rec[:3].tobytes()
        ctx.upload_scene(nodes, tris, mats)
        whole = ctx.trace_paths_into(rec.copy())
        # a zero-byte call, from the host and from the device
        assert ctx.trace_paths_into(rec[:0].copy()).shape == (0,)
        assert ctx.trace_paths_into(torch.zeros((0, 12), device="cuda:0")).shape == (0, 12)
        # invalid records: a NaN or an inf in each of the six components, budgets of 0, 1025 and 0xFFFFFFFF — among valid ones
        hit = np.flatnonzero(whole["segments"] > 1)[:16]
        bad = rec[hit].copy()
        for k in range(6):
            bad["org" if k < 3 else "dir"][k, k % 3] = np.nan
            bad["org" if k < 3 else "dir"][6 + k, k % 3] = np.inf if k % 2 else -np.inf
        bad["max_bounces"][12], bad["max_bounces"][13], bad["max_bounces"][14] = 0, 1025, 0xFFFFFFFF
        for records, where in ((ctx.trace_paths_into(bad.copy()), "host"), (from_device(native, ctx.trace_paths_into(on_device(bad))), "device")):
            check_ins(records, bad, where)
            assert not pq.bits(records["radiance"][:15]).any() and not records["segments"][:15].any(), where
            assert records[15:].tobytes() == whole[hit][15:].tobytes(), where
        # the largest legal budget is legal
        top = rec[hit][:2].copy()
        top["max_bounces"] = native.PATH_MAX_BOUNCES
        assert (ctx.trace_paths_into(top)["segments"] >= whole["segments"][hit][:2]).all()
        # seed 0: xorshift32 stays 0, every rand() is 0 — a path like any other, and the render's for a pixel whose state were 0 (same call twice: same bytes)
        zero = rec.copy()
        zero["seed"] = 0
        a, b = ctx.trace_paths_into(zero.copy()), ctx.trace_paths_into(zero.copy())
        assert a.tobytes() == b.tobytes() and (a["segments"] >= 1).all() and (a["segments"] <= 8).all()
        assert out_bytes(a[whole["segments"] == 1]) == out_bytes(whole[whole["segments"] == 1])  # a camera ray that misses draws nothing
        # byte counts that are no whole number of records, through the C call: dst untouched
        buf = rec[:2].copy()
        for nbytes in (47, 49, 95):
            rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_RAY_PATHS, buf.ctypes.data_as(ctypes.c_void_p), nbytes)
            assert rc == native.ERR_INVALID and b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h) and b"rvpt_ray_path" in ctx._L.rvpt_hip_last_error(ctx._h)
            assert buf.tobytes() == rec[:2].tobytes()
        # a successful query leaves last_error as it was
        ctx.trace_paths_into(rec[:1].copy())
        assert b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h)
        # a view that starts 4 bytes in: device records need 16-byte alignment; memory untouched
        flat = on_device(rec[:8]).reshape(-1)
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="16-byte alignment") as e:
            ctx.trace_paths_into(flat[1:1 + 12 * 5].reshape(5, 12))
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        # trace_paths builds the records itself: scalars or one value per ray
        k = int(hit[0])
        out = ctx.trace_paths(rec["org"][k], rec["dir"][k], int(rec["seed"][k]), 8)
        assert out.dtype == native.RAY_PATH_DTYPE and out_bytes(out) == out_bytes(whole[k:k + 1])
        out = ctx.trace_paths(rec["org"][:70], rec["dir"][:70], rec["seed"][:70], np.full(70, 8))
        assert out_bytes(out) == out_bytes(whole[:70])
        # the empty scene: the miss radiance of dir and one segment — the integrator's value itself
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        empty = ctx.trace_paths_into(rec.copy())
        assert (empty["segments"] == 1).all() and pq.same_bits(empty["radiance"], pq.miss_radiance(rec["dir"]))
        empty_bad = ctx.trace_paths_into(bad.copy())
        assert not empty_bad["segments"][:15].any() and empty_bad["segments"][15] == 1
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["bvh", "brute"])
def test_a_path_query_leaves_frames_untouched(native, oracle, showcase, showcase_cam, kind):
    """Two accumulated frames, a query, a third frame: image, stats, the timing's dispatch count, launch_info and cull_info equal a context that never asked"""
    from rvpt_amd import RenderSettings
    rec = records_for(oracle, showcase_cam, 0, 0, 8)
    out = []
    for asks in (False, True):
        ctx = make_context(native, kind, showcase, native.COUNT_SEGMENTS | native.TIMING)
        try:
            if asks:
                ctx.trace_paths_into(rec[:300].copy())  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), showcase_cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.trace_paths_into(rec.copy())  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((pq.bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info()))
        finally:
            ctx.close()
    assert out[0] == out[1]


def test_the_renderers_defaults_are_a_frames(native, oracle, showcase_cam):
    """RVPT.trace_paths without seed and budget: seed[i] = wang_hash(i) + current frame, the render settings' budget"""
    from rvpt_amd import RVPT, scene
    from rvpt_amd.renderer import wang_hash
    tris, mats = scene.materials_showcase_scene()
    r = RVPT(W, H, device=0, traversal="bvh")
    try:
        with pytest.raises(RuntimeError, match="before initialize"):
            r.trace_paths(np.zeros(3), np.ones(3))
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        rec = records_for(oracle, showcase_cam, 0, 0, 8)[:200]
        r.render_settings.current_frame, r.render_settings.max_bounces = 4, 3
        got = r.trace_paths(rec["org"], rec["dir"])
        assert got["seed"].tolist() == [(oracle.wang_hash(i) + 4) & 0xFFFFFFFF for i in range(200)] and (got["max_bounces"] == 3).all()
        want = r.context.trace_paths(rec["org"], rec["dir"], wang_hash(np.arange(200, dtype=np.uint32)) + np.uint32(4), 3)
        assert got.tobytes() == want.tobytes() and (got["segments"] > 1).any()
        explicit = r.trace_paths(rec["org"], rec["dir"], seed=rec["seed"], max_bounces=8)
        assert (explicit["seed"] == rec["seed"]).all() and (explicit["max_bounces"] == 8).all()
    finally:
        r.shutdown()
