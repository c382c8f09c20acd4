"""Path queries by integrator on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_RAY_PATHS_MODE(m) (Context.trace_paths_into(records, mode=m)) against oracle.render
with modes=(m, m, m, m).  The records are the ones a frame's pixels would ask with (tests/_path_query.py): the integrator receives only the ray and the RNG state,
so they serve every render mode.  Everything runs at 48 x 32 — 1536 records, 12 runs of 128, several waves per work-group and a last partial run — and whole
images and whole records are compared, bit for bit: no pixel or record is left out of any comparison."""
import ctypes

import numpy as np
import pytest

import _guarded_pose as gp
import _path_query as pq
import _skin
from _util import identity_camera, scene_by_name
from test_path_query import (H, W, camera_at, chain_scene, check_ins, from_device, kernel_constant, make_context, on_device, out_bytes, out_view, records_for)

pytestmark = pytest.mark.gpu
RENDER_MODES = list(range(9))  # binary, color, depth, normal, Utah, ambient occlusion, Appel, Whitted, Cook


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


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


_renders = {}


def render_of(oracle, scene3, cam, traversal, mode, camera, frame, budget):
    """oracle.render's (image, stats) of the frame, once per argument set and never changed"""
    tris, mats, nodes = scene3
    key = (tris.tobytes(), None if nodes is None else np.asarray(nodes).tobytes(), cam.tobytes(), traversal, mode, camera, frame, budget)
    if key not in _renders:
        settings = oracle.settings_bytes(max_bounces=budget, aa=1, current_frame=frame, camera_mode=camera, modes=(mode,) * 4)
        img, stats = oracle.render(settings, cam, nodes if traversal == 0 else None, tris, mats, W, H, traversal)
        img.setflags(write=False)
        _renders[key] = (img, stats)
    return _renders[key]


def check_against_render(oracle, native, ctx, rec, cam, scene3, traversal, mode, camera, frame, budget, what):
    """host records and device records: the oracle's image and segment count, and each other's bytes; the in fields unchanged over poisoned out fields"""
    img, stats = render_of(oracle, scene3, cam, traversal, mode, camera, frame, budget)
    assert (rec["segments"] == 0xCDCDCDCD).all()  # (records_for poisons the out fields)
    host = ctx.trace_paths_into(rec.copy(), mode=mode)
    dev = from_device(native, ctx.trace_paths_into(on_device(rec), mode=mode))
    for got, where in ((host, "host records"), (dev, "device records")):
        check_ins(got, rec, f"{what}, {where}")
        image = pq.expected_image(got["radiance"], frame, W, H)
        print(f"{what}, {where}: {int((pq.bits(image) != pq.bits(img[..., :3])).any(axis=-1).sum())} of {W * H} pixels differ, "
              f"segments {int(got['segments'].sum(dtype=np.uint64))} against {int(stats[0])}")
        assert pq.same_bits(image, img[..., :3]), f"{what}, {where}: {pq.first_difference(image, img[..., :3])}"
        assert int(got["segments"].sum(dtype=np.uint64)) == int(stats[0]), (what, where)
    assert out_bytes(host) == out_bytes(dev), what
    return host


def allowed_segments(mode, budget):
    """the segment counts a valid record may come back with (integrators.glsl, shade_generic): modes 0-4 ask once; ambient occlusion asks once and, at a hit,
    once per sample; Appel asks once and, at a hit, one shadow query; Whitted and Cook trace up to `budget` main segments and end on a Lambert hit with one
    more query (the shadow ray / the last diffuse bounce)"""
    if mode <= 4:
        return {1}
    if mode == 5:
        return {1, 1 + budget}
    if mode == 6:
        return {1, 2}
    return set(range(1, budget + 2))


# ---- 1. parity with the reference integrator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
@pytest.mark.parametrize("mode", RENDER_MODES)
def test_radiance_is_the_reference_integrators(native, oracle, showcase, showcase_cam, mode, kind):
    """48 x 32 on the showcase scene (mirror, glass, emitter), pinhole camera, budgets 1, 2 and 8, frames 0 and 5.  3. The per-record segment counts are the
    ones the integrator allows, and every allowed value is attained (Whitted, Cook: one segment, and more than one)."""
    ctx = make_context(native, kind, showcase)
    try:
        for frame in (0, 5):
            for budget in (1, 2, 8):
                rec = records_for(oracle, showcase_cam, 0, frame, budget)
                got = check_against_render(oracle, native, ctx, rec, showcase_cam, showcase, 1 if kind == "brute" else 0, mode, 0, frame, budget,
                                           f"render mode {mode} {kind} frame {frame} budget {budget}")
                seen, allowed = set(got["segments"].tolist()), allowed_segments(mode, budget)
                assert seen <= allowed, (mode, budget, sorted(seen - allowed))
                if mode <= 6:
                    assert seen == allowed, (mode, budget, sorted(seen))
                else:
                    assert 1 in seen and max(seen) > 1, (mode, budget, sorted(seen))
    finally:
        ctx.close()


# ---- 2. directions that are not unit length ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
@pytest.mark.parametrize("camera", [1, 2])
@pytest.mark.parametrize("mode", [2, 6])
def test_directions_that_are_not_unit_length(native, oracle, showcase, showcase_cam, mode, camera, kind):
    """depth divides by |d| and Appel normalises d: the orthographic camera's direction is a matrix column, the spherical camera's a matrix product"""
    ctx = make_context(native, kind, showcase)
    try:
        for frame in (0, 5):
            for budget in (1, 2, 8):
                rec = records_for(oracle, showcase_cam, camera, frame, budget)
                got = check_against_render(oracle, native, ctx, rec, showcase_cam, showcase, 1 if kind == "brute" else 0, mode, camera, frame, budget,
                                           f"render mode {mode} camera {camera} {kind} frame {frame} budget {budget}")
                assert set(got["segments"].tolist()) <= allowed_segments(mode, budget)
        lengths = np.linalg.norm(rec["dir"].astype(np.float64), axis=1)
        assert camera != 2 or (np.abs(lengths - 1.0) > 0).any()  # (bits away from unit length, which is all the integrators need to differ)
    finally:
        ctx.close()


# ---- 4. the context's own frame ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
@pytest.mark.parametrize("mode", RENDER_MODES)
def test_radiance_is_the_contexts_own_frame(native, oracle, showcase, showcase_cam, mode, kind):
    """Same records, same context: the frame with that mode in all four quadrants is 0 + radiance (scaled as a first frame is), and its segment count is the
    records' sum"""
    from rvpt_amd import RenderSettings
    ctx = make_context(native, kind, showcase, native.COUNT_SEGMENTS)
    try:
        for frame in (0, 5):
            rec = records_for(oracle, showcase_cam, 0, frame, 8)
            got = ctx.trace_paths_into(rec.copy(), mode=mode)
            before = ctx.stats()[0]
            ctx.set_frame(RenderSettings(max_bounces=8, aa=1, current_frame=frame, top_left_render_mode=mode, top_right_render_mode=mode, bottom_left_render_mode=mode,
                                         bottom_right_render_mode=mode).pack(), showcase_cam)
            ctx.dispatch()
            img = ctx.read()
            image = pq.expected_image(got["radiance"], frame, W, H)
            assert pq.same_bits(image, img[..., :3]), f"render mode {mode} {kind} frame {frame}: {pq.first_difference(image, img[..., :3])}"
            assert ctx.stats()[0] - before == int(got["segments"].sum(dtype=np.uint64))
            ctx.write_accum(np.zeros((H, W, 4), np.float32))  # (the next frame of this loop starts from nothing, as the oracle's)
    finally:
        ctx.close()


# ---- 5. mode 9 is format 3 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
def test_mode_nine_is_format_three(native, oracle, showcase, showcase_cam, kind):
    """Format 25 through the C call against format 3 through the C call: identical records, from host and from device memory, budgets 1 and 8"""
    ctx = make_context(native, kind, showcase)
    try:
        assert native.format_ray_paths_mode(9) == 25
        for budget in (1, 8):
            rec = records_for(oracle, showcase_cam, 0, 0, budget)
            answers = []
            for fmt in (native.FORMAT_RAY_PATHS, 25):
                host = rec.copy()
                assert ctx._L.rvpt_hip_read(ctx._h, fmt, host.ctypes.data_as(ctypes.c_void_p), host.nbytes) == 0
                dev = on_device(rec)
                assert ctx._L.rvpt_hip_read(ctx._h, fmt, ctypes.c_void_p(dev.data_ptr()), rec.nbytes) == 0
                answers += [host.tobytes(), from_device(native, dev).tobytes()]
            assert len(set(answers)) == 1 and answers[0] != rec.tobytes()
            assert ctx.trace_paths_into(rec.copy(), mode=9).tobytes() == answers[0] == ctx.trace_paths_into(rec.copy()).tobytes()
    finally:
        ctx.close()


# ---- 6. batch independence --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["brute", "bvh"])
@pytest.mark.parametrize("mode", [5, 7, 8])
def test_a_records_answer_does_not_depend_on_its_batch(native, oracle, showcase, showcase_cam, mode, kind):
    """What phase state leaking between records through regeneration would break.  One call, a seeded shuffle, and batches of 1, 63, 64, 65, 127 and 129
    records over the shuffle: every record's 16 out bytes are the one-call answer's."""
    ctx = make_context(native, kind, showcase)
    try:
        rec = records_for(oracle, showcase_cam, 0, 0, 8)
        whole = ctx.trace_paths_into(rec.copy(), mode=mode)
        assert len(set(whole["segments"].tolist())) > 1  # (records of different lengths share waves)
        order = np.random.RandomState(23 + mode).permutation(rec.shape[0])
        shuffled = ctx.trace_paths_into(rec[order].copy(), mode=mode)
        assert out_view(shuffled).tobytes() == out_view(whole)[order].tobytes()
        for size in (1, 63, 64, 65, 127, 129):
            parts = [ctx.trace_paths_into(rec[order][at:at + size].copy(), mode=mode) for at in range(0, rec.shape[0], size)]
            got = np.concatenate(parts)
            assert out_view(got).tobytes() == out_view(whole)[order].tobytes(), size
            check_ins(got, rec[order], f"batches of {size}")
        dev_parts = [from_device(native, ctx.trace_paths_into(on_device(rec[order][at:at + 129]), mode=mode)) for at in range(0, rec.shape[0], 129)]
        assert np.concatenate(dev_parts).tobytes() == whole[order].tobytes()
    finally:
        ctx.close()


# ---- 7. the other two walks and deep trees ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [5, 7])
def test_inside_the_cornell_box_on_the_wide_walk(native, oracle, cornell, cornell_cam, mode):
    """9164 triangles from inside the box, budget 8: every pixel hits.  The 4-wide walk through HBM-resident nodes."""
    assert cornell[0].shape[0] == 9164
    ctx = make_context(native, "bvh", cornell)
    try:
        rec = records_for(oracle, cornell_cam, 0, 0, 8)
        got = check_against_render(oracle, native, ctx, rec, cornell_cam, cornell, 0, mode, 0, 0, 8, f"cornell, render mode {mode}")
        assert (got["segments"] > 1).all() and (mode != 5 or (got["segments"] == 9).all())
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", [5, 7])
def test_inside_the_cornell_box_on_a_device_built_tree(native, oracle, cornell, cornell_cam, mode):
    """The same on a context whose LBVH tree the device built from shuffled triangles: the oracle gets the numpy statement of that tree"""
    from rvpt_amd import scene
    tris, mats, _ = cornell
    tris = tris[np.random.RandomState(2).permutation(tris.shape[0])]
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, "lbvh") == "lbvh"
        nodes, perm = scene.build_lbvh(tris)[:2]
        rec = records_for(oracle, cornell_cam, 0, 0, 8)
        check_against_render(oracle, native, ctx, rec, cornell_cam, (tris[perm], mats, nodes), 0, mode, 0, 0, 8, f"cornell built by lbvh, render mode {mode}")
    finally:
        ctx.close()


@pytest.mark.parametrize("walk", ["wide", "binary"])
def test_whitted_through_the_overflow_stack(native, oracle, monkeypatch, walk):
    """The mirrored chain (tests/test_path_query.py: 47 slots on the wide walk, 48 on the binary one, past the 8 a lane keeps in LDS): mode 7 through the global
    columns of path_bvh4 and, on a laboratory context that holds no wide form, through path_bvh2 — the binary walk."""
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
        rec = records_for(oracle, cam, 0, 0, 8)
        got = check_against_render(oracle, native, ctx, rec, cam, scene3, 0, 7, 0, 0, 8, f"chain, {walk} walk, render mode 7")
        assert (got["segments"] > 1).sum() > 50
        if walk == "binary":  # the hit-only instance of the binary walk too
            check_against_render(oracle, native, ctx, rec, cam, scene3, 0, 3, 0, 0, 8, "chain, binary walk, render mode 3")
    finally:
        ctx.close()


# ---- 8. after an update -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["skin", "guarded pose"])
def test_ambient_occlusion_after_an_update(native, oracle, form):
    """Mode 5 on the scene as a skin update / a rebuilding guarded pose update left it, against oracle.render on the model's tree"""
    from rvpt_amd import scene
    cam = identity_camera(W / H)
    rec = records_for(oracle, cam, 0, 0, 8)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        if form == "skin":
            tris, mats, nodes = scene_by_name("default")
            ctx.upload_scene(nodes, tris, mats)
            before = ctx.trace_paths_into(rec.copy(), mode=5)
            weights, matrices = _skin.weights(tris, 6), _skin.bones(tris, 6, 0.4)
            skinned = scene.skin_triangles(tris, weights, matrices)
            ctx.bind_skin(weights)
            ctx.skin(matrices)
            model = (skinned, mats, scene.refit_bvh(nodes, skinned))
        else:
            tris, mats = scene.default_scene()
            assert ctx.build_scene(tris, mats, "lbvh") == "lbvh"
            before = ctx.trace_paths_into(rec.copy(), mode=5)
            first, count = gp.part_of(tris.shape[0])
            moves = [gp.turned(tris, first, count, 90.0)]
            step = gp.step(gp.built(tris, "lbvh"), moves, 1.02, "lbvh")
            assert step.rebuilt and ctx.pose_parts(moves, rebuild_above=1.02).rebuilt
            model = (step.state.current[step.state.perm], mats, step.state.nodes)
        got = check_against_render(oracle, native, ctx, rec, cam, model, 0, 5, 0, 0, 8, f"render mode 5 after a {form} update")
        assert out_bytes(got) != out_bytes(before) and set(got["segments"].tolist()) == {1, 9}
    finally:
        ctx.close()


# ---- 9. invalid records, the empty scene, errors ----------------------------------------------------------------------------------------------------------
def test_invalid_records_the_empty_scene_and_the_errors(native, oracle, showcase, showcase_cam):
    import torch
    tris, mats, nodes = showcase
    rec = records_for(oracle, showcase_cam, 0, 0, 8)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        # no scene yet
        untouched = rec[:3].copy()
        for mode in (0, 5, 7):
            with pytest.raises(native.NativeError, match="path query before any full upload_scene") as e:
                ctx.trace_paths_into(untouched, mode=mode)
            assert e.value.code == native.ERR_INVALID and untouched.tobytes() == rec[:3].tobytes()
        ctx.upload_scene(nodes, tris, mats)
        for mode in (0, 5, 7):
            whole = ctx.trace_paths_into(rec.copy(), mode=mode)
            # a zero-byte call, from the host and from the device
            assert ctx.trace_paths_into(rec[:0].copy(), mode=mode).shape == (0,)
            assert ctx.trace_paths_into(torch.zeros((0, 12), device="cuda:0"), mode=mode).shape == (0, 12)
            # format 3's invalid records: a NaN or an inf in each of the six components, budgets of 0, 1025 and 0xFFFFFFFF — among valid ones
            hit = np.flatnonzero(whole["segments"] > 1)[:16] if mode != 0 else np.flatnonzero(whole["radiance"][:, 0] == 1.0)[:16]
            assert hit.shape[0] == 16
            bad = rec[hit].copy()
            for k in range(6):
                bad["org" if k < 3 else "dir"][k, k % 3] = np.nan
                bad["org" if k < 3 else "dir"][6 + k, k % 3] = np.inf if k % 2 else -np.inf
            bad["max_bounces"][12], bad["max_bounces"][13], bad["max_bounces"][14] = 0, 1025, 0xFFFFFFFF
            for records, where in ((ctx.trace_paths_into(bad.copy(), mode=mode), "host"), (from_device(native, ctx.trace_paths_into(on_device(bad), mode=mode)), "device")):
                check_ins(records, bad, where)
                assert not pq.bits(records["radiance"][:15]).any() and not records["segments"][:15].any(), (mode, where)
                assert records[15:].tobytes() == whole[hit][15:].tobytes(), (mode, where)
            # the largest legal budget is legal (1024 occlusion samples; the hit-only modes ignore it)
            top = rec[hit][:2].copy()
            top["max_bounces"] = native.PATH_MAX_BOUNCES
            assert (ctx.trace_paths_into(top, mode=mode)["segments"] == {0: 1, 5: 1025}[mode]).all() if mode != 7 else (ctx.trace_paths_into(top, mode=mode)["segments"] >= 2).all()
            # byte counts that are no whole number of records, through the C call: dst untouched
            buf = rec[:2].copy()
            for nbytes in (47, 49):
                rc = ctx._L.rvpt_hip_read(ctx._h, native.format_ray_paths_mode(mode), buf.ctypes.data_as(ctypes.c_void_p), nbytes)
                assert rc == native.ERR_INVALID and b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h) and b"rvpt_ray_path" in ctx._L.rvpt_hip_last_error(ctx._h)
                assert buf.tobytes() == rec[:2].tobytes()
            # a successful query leaves last_error as it was
            ctx.trace_paths_into(rec[:1].copy(), mode=mode)
            assert b"multiple" in ctx._L.rvpt_hip_last_error(ctx._h)
            # a view that starts 4 bytes in: device records need 16-byte alignment; memory untouched
            flat = on_device(rec[:8]).reshape(-1)
            keep = flat.clone()
            with pytest.raises(native.NativeError, match="16-byte alignment") as e:
                ctx.trace_paths_into(flat[1:1 + 12 * 5].reshape(5, 12), mode=mode)
            assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        # another format value: Hart's would-be 26, 27, and 15 below the range — the unknown format of a frame read, dst untouched
        buf = rec[:2].copy()
        for fmt in (26, 27, 15):
            rc = ctx._L.rvpt_hip_read(ctx._h, fmt, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes)
            assert rc == native.ERR_INVALID and f"unknown format {fmt}".encode() in ctx._L.rvpt_hip_last_error(ctx._h)
            assert buf.tobytes() == rec[:2].tobytes()
        # the empty scene: the integrator's miss value and one segment, for every valid record — the oracle's frame of a scene without triangles
        none = np.zeros((0, 16), np.float32)
        ctx.upload_scene(None, none, mats)
        for mode in RENDER_MODES:
            got = check_against_render(oracle, native, ctx, rec, showcase_cam, (none, mats, None), 1, mode, 0, 0, 8, f"empty scene, render mode {mode}")
            assert (got["segments"] == 1).all()
            empty_bad = ctx.trace_paths_into(bad.copy(), mode=mode)
            assert not empty_bad["segments"][:15].any() and not pq.bits(empty_bad["radiance"][:15]).any() and empty_bad["segments"][15] == 1
    finally:
        ctx.close()


# ---- 10. a query leaves frames untouched ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bvh", "brute"])
def test_a_path_query_leaves_frames_untouched(native, oracle, showcase, showcase_cam, kind):
    """Two accumulated frames, a Whitted query, a third frame: image, stats, the timing's dispatch count, launch_info and cull_info equal a context that never
    asked"""
    from rvpt_amd import RenderSettings
    rec = records_for(oracle, showcase_cam, 0, 0, 8)
    out = []
    for asks in (False, True):
        ctx = make_context(native, kind, showcase, native.COUNT_SEGMENTS | native.TIMING)
        try:
            if asks:
                ctx.trace_paths_into(rec[:300].copy(), mode=7)  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), showcase_cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.trace_paths_into(rec.copy(), mode=7)  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((pq.bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info()))
        finally:
            ctx.close()
    assert out[0] == out[1]


# ---- 11. the wrappers -------------------------------------------------------------------------------------------------------------------------------------
def test_the_renderer_takes_the_mode_by_name(native, oracle, showcase_cam):
    """RVPT.trace_paths(mode="ao") is Context.trace_paths(..., mode=5); None is integrator_Kajiya, as before"""
    from rvpt_amd import RVPT, scene
    from rvpt_amd.renderer import wang_hash
    tris, mats = scene.materials_showcase_scene()
    r = RVPT(W, H, device=0, traversal="bvh")
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        rec = records_for(oracle, showcase_cam, 0, 0, 8)[:200]
        r.render_settings.current_frame, r.render_settings.max_bounces = 4, 3
        seeds = wang_hash(np.arange(200, dtype=np.uint32)) + np.uint32(4)
        got = r.trace_paths(rec["org"], rec["dir"], mode="ao")
        want = r.context.trace_paths(rec["org"], rec["dir"], seeds, 3, mode=5)
        assert got.tobytes() == want.tobytes() and set(got["segments"].tolist()) == {1, 4}
        assert r.trace_paths(rec["org"], rec["dir"], mode=5).tobytes() == want.tobytes()
        kajiya = r.context.trace_paths(rec["org"], rec["dir"], seeds, 3)
        assert r.trace_paths(rec["org"], rec["dir"]).tobytes() == kajiya.tobytes() == r.trace_paths(rec["org"], rec["dir"], mode="kajiya").tobytes()
        assert kajiya.tobytes() != want.tobytes()
    finally:
        r.shutdown()
