"""Moving geometry on the GPU: the update form of rvpt_hip_upload_scene (Context.update_triangles) refits the tree on the device.  Everything here is bit-exact:
after an update the context renders what a fresh context given upload_scene(refit_bvh(nodes, t), t, mats) renders, which is what the CPU oracle renders on
that tree."""
import os

import numpy as np
import pytest

from _util import identity_camera, scene_by_name
from test_gpu_parity import _chain_bvh, _loosen_boxes, oracle_frames

pytestmark = pytest.mark.gpu

PHASES = (0.7, 1.9, 3.4)


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def extent(tris):
    return float(np.ptp(tris.reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3), axis=0).max())


def flags_of(native, traversal, extra=0):
    return extra | {"bvh": native.TRAVERSAL_BVH, "brute": native.TRAVERSAL_BRUTE, "bvh_ordered": native.TRAVERSAL_BVH_ORDERED}[traversal]


def render(ctx, cam, frames, aa=1, batch=False, max_bounces=8):
    """frames f = 0 .. frames - 1 from a restarted accumulation (one launch each, or one batched launch); the image after the last"""
    from rvpt_amd import RenderSettings
    if batch:
        ctx.set_frame(RenderSettings(max_bounces=max_bounces, aa=aa, current_frame=0).pack(), cam)
        ctx.dispatch_frames(frames)
    else:
        for f in range(frames):
            ctx.set_frame(RenderSettings(max_bounces=max_bounces, aa=aa, current_frame=f).pack(), cam)
            ctx.dispatch()
    return ctx.read()


def terrain64():
    from rvpt_amd import native as n, scene
    tris, mats = scene.heightfield_scene(64)
    nodes, idx = n.build_bvh(tris)
    return tris[idx], mats, nodes


def scene_and_camera(name, W, H):
    from rvpt_amd import Camera
    sc = terrain64() if name == "terrain64" else scene_by_name(name)
    c = Camera(W / H)
    if name == "cornell":
        c.translation = np.array([0.0, 2.0, -1.9])
    elif name == "terrain64":
        c.translation = np.array([0.0, 2.5, -5.0])
        c.rotation = np.array([0.0, 25.0, 0.0])
    else:
        return sc, identity_camera(W / H)
    return sc, c.get_data()


IDENTITY = [("bvh", 0, 11), ("bvh_ordered", 0, 3), ("bvh", "per_lane", 3), ("brute", 0, 6)]


@pytest.mark.parametrize("traversal,extra,variant", IDENTITY)
def test_update_with_the_same_triangles_changes_nothing(native, traversal, extra, variant):
    """upload, render, update_triangles(same), render again from frame 0: the same image, the same segment counts, the same kernel path and culls."""
    W, H = 160, 96
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS | (native.BVH_PER_LANE if extra == "per_lane" else 0))
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if traversal != "brute" else None, tris, mats)
        first = render(ctx, cam, 2, aa=2)
        s0, launch0, cull0 = ctx.stats(), ctx.launch_info()[:3], ctx.cull_info()
        assert launch0[2] == variant
        ctx.update_triangles(tris)
        again = render(ctx, cam, 2, aa=2)
        s1 = ctx.stats()
        assert np.array_equal(bits(first), bits(again))
        assert (s1[0] - s0[0], s1[1] - s0[1]) == s0
        assert ctx.launch_info()[:3] == launch0 and ctx.cull_info() == cull0
        if traversal == "brute":
            assert cull0 & 0x57 == 0x57  # rectangles, bounce table, block rounds, leaf boxes, the lean instance: the packet kernel with all its culls
    finally:
        ctx.close()


DEFORM = [
    # scene, traversal, extra flag, W, H, aa, batched, kernel path
    ("default", "bvh", 0, 96, 64, 1, False, 11),        # the LDS-resident wide walk
    ("cornell", "bvh", 0, 96, 64, 1, False, 10),        # the HBM-resident 4-wide walk
    ("terrain64", "bvh", 0, 96, 64, 1, False, 10),
    ("cornell", "bvh_ordered", 0, 80, 48, 1, False, 2),  # nearer child first, binary nodes
    ("cornell", "bvh", "per_lane", 80, 48, 1, False, 2),
    ("default", "bvh", 0, 80, 48, 2, False, 11),
    ("cornell", "bvh", 0, 80, 48, 1, True, 10),         # one launch of two frames
    ("default", "bvh", "per_lane", 80, 48, 2, True, 3),
]


@pytest.mark.parametrize("name,traversal,extra,W,H,aa,batch,variant", DEFORM)
def test_deformed_geometry_renders_as_a_fresh_upload_of_the_refit_tree(native, oracle, name, traversal, extra, W, H, aa, batch, variant):
    """Three phases of a smooth deformation (a tenth of the scene's extent) applied one after another to ONE context; after each, two frames equal (a) a fresh
    context given the numpy refit of the tree and (b) the oracle on that tree, segment counts included."""
    from rvpt_amd import scene
    (tris, mats, nodes), cam = scene_and_camera(name, W, H)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS | (native.BVH_PER_LANE if extra == "per_lane" else 0))
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes, tris, mats)
        still = render(ctx, cam, 2, aa=aa, batch=batch)
        info = ctx.launch_info()
        assert info[2] == variant
        seen = ctx.stats()
        for phase in PHASES:
            moved = scene.wobble(tris, phase, 0.1 * extent(tris))
            refit = scene.refit_bvh(nodes, moved)
            ctx.update_triangles(moved)
            got = render(ctx, cam, 2, aa=aa, batch=batch)
            now = ctx.stats()
            assert ctx.launch_info()[1:3] == info[1:3]  # topology-only state: the same kernel path, the same LDS
            fresh = native.Context(W, H, 0, 0, 1, fl)
            try:
                fresh.upload_scene(refit, moved, mats)
                want = render(fresh, cam, 2, aa=aa, batch=batch)
                want_stats = fresh.stats()
            finally:
                fresh.close()
            ref, seg = oracle_frames(oracle, (moved, mats, refit), cam, W, H, traversal, [0, 1], aa=aa)
            assert not np.array_equal(bits(got), bits(still)), f"phase {phase}: the geometry did not move"
            assert np.array_equal(bits(got), bits(want)), f"phase {phase}: update != fresh upload of the refit tree"
            assert np.array_equal(bits(got), bits(ref[1])), f"phase {phase}: update != oracle"
            assert (now[0] - seen[0], now[1] - seen[1]) == want_stats and want_stats[0] == seg
            seen = now
    finally:
        ctx.close()


@pytest.mark.parametrize("culls", ["on", "off"])
def test_deformed_geometry_brute_force(native, oracle, monkeypatch, culls):
    """Brute-force contexts: prepared records, the bounce cull's table, the scene scale and the leaf boxes follow the vertices; against the oracle's brute-force
    variant with every cull of the packet kernel on, and with all of them off."""
    from rvpt_amd import scene
    if culls == "off":
        for k in ("RVPT_HIP_PACKETS_CULL", "RVPT_HIP_PACKETS_BOUNCE_CULL", "RVPT_HIP_PACKETS_BOX_CULL"):
            monkeypatch.setenv(k, "0")
    W, H = 96, 64
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    ctx = native.Context(W, H, 0, 0, 1, native.COUNT_SEGMENTS)
    try:
        ctx.upload_scene(None, tris, mats)
        render(ctx, cam, 1)
        cull0 = ctx.cull_info()
        assert ctx.launch_info()[2] == 6 and ((cull0 & 0x13) == 0x13) == (culls == "on")
        seen = ctx.stats()
        for phase in PHASES:
            moved = scene.wobble(tris, phase, 0.1 * extent(tris))
            ctx.update_triangles(moved)
            got = render(ctx, cam, 2, aa=2)
            now = ctx.stats()
            assert ctx.cull_info() == cull0
            ref, seg = oracle_frames(oracle, (moved, mats, nodes), cam, W, H, "brute", [0, 1], aa=2)
            assert np.array_equal(bits(got), bits(ref[1])), f"phase {phase}: update != oracle (culls {culls})"
            assert now[0] - seen[0] == seg
            seen = now
        ctx.update_triangles(scene.wobble(tris, 0.4, 0.1 * extent(tris)))
        ctx.set_frame(__import__("rvpt_amd").RenderSettings(current_frame=0).pack(), cam)
        ctx.dispatch_frames(5)  # a batched launch: the sky list is rebuilt for the moved triangles' rectangles
        got = ctx.read()
        ref, _ = oracle_frames(oracle, (scene.wobble(tris, 0.4, 0.1 * extent(tris)), mats, nodes), cam, W, H, "brute", [0, 1, 2, 3, 4])
        assert np.array_equal(bits(got), bits(ref[4]))
    finally:
        ctx.close()


def _two_leaf_tree(tris):
    """root + two leaves of ~n / 2 triangles each: leaves far beyond the builder's eight"""
    n = tris.shape[0]
    nodes = np.zeros(3, dtype=np.dtype([("first", "<u4"), ("count", "<u4"), ("bounds", "<f4", (6,))]))
    nodes[0] = (1, 0, [0] * 6)
    nodes[1] = (0, n // 2, [0] * 6)
    nodes[2] = (n // 2, n - n // 2, [0] * 6)
    return nodes


@pytest.mark.parametrize("shape", ["single_leaf", "chain", "big_leaves", "degenerate"])
@pytest.mark.parametrize("traversal", ["bvh", "bvh_ordered"])
def test_shapes_of_tree(native, oracle, shape, traversal):
    """A tree that is one leaf (no wide form), the deepest chain the reference's stack walks (64 levels = 64 refit launches), leaves of 71 and 72 triangles, and a
    deformation that collapses triangles to a segment and to a point."""
    from rvpt_amd import scene
    W, H = 80, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    if shape == "single_leaf":
        tris = tris[:6].copy()
        nodes = np.zeros(1, dtype=native.NODE_DTYPE)
        nodes[0] = (0, 6, [0] * 6)
    elif shape == "chain":
        tris = tris[:64].copy()
        nodes = _chain_bvh(tris)
    elif shape == "big_leaves":
        nodes = _two_leaf_tree(tris)
    nodes = scene.refit_bvh(nodes, tris)
    moved = scene.wobble(tris, 2.2, 0.1 * extent(tris))
    if shape == "degenerate":
        moved[3, 4:7] = moved[3, 0:3]                           # a segment
        moved[40, 4:7] = moved[40, 8:11] = moved[40, 0:3]       # a point
    refit = scene.refit_bvh(nodes, moved)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS)
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes, tris, mats)
        render(ctx, cam, 1)
        seen = ctx.stats()
        ctx.update_triangles(moved)
        got = render(ctx, cam, 2, aa=2)
        now = ctx.stats()
    finally:
        ctx.close()
    ref, seg = oracle_frames(oracle, (moved, mats, refit), cam, W, H, traversal, [0, 1], aa=2)
    assert np.array_equal(bits(got), bits(ref[1])) and now[0] - seen[0] == seg


def test_loose_boxes_become_tight(native, oracle):
    """A caller's tree whose inner boxes do not contain their children culls where the reference would (test_wide_tree_walk_equals_the_binary_walk); after an update
    — even with the same vertices — the boxes are the refit's, i.e. tight, and the image is the valid tree's, which differs."""
    from rvpt_amd import scene
    W, H = 128, 80
    (tris, mats, nodes), cam = scene_and_camera("cornell", W, H)
    loose = _loosen_boxes(nodes, 5)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(loose, tris, mats)
        img_loose = render(ctx, cam, 1)
        ctx.update_triangles(tris)
        img_tight = render(ctx, cam, 1)
        moved = scene.wobble(tris, 1.0, 0.1 * extent(tris))
        ctx.update_triangles(moved)
        img_moved = render(ctx, cam, 1)
    finally:
        ctx.close()
    ref_loose, _ = oracle_frames(oracle, (tris, mats, loose), cam, W, H, "bvh", [0])
    ref_tight, _ = oracle_frames(oracle, (tris, mats, nodes), cam, W, H, "bvh", [0])
    ref_moved, _ = oracle_frames(oracle, (moved, mats, scene.refit_bvh(loose, moved)), cam, W, H, "bvh", [0])
    assert scene.refit_bvh(loose, tris).tobytes() == np.ascontiguousarray(nodes).tobytes()
    assert np.array_equal(bits(img_loose), bits(ref_loose[0])) and not np.array_equal(bits(ref_loose[0]), bits(ref_tight[0]))
    assert np.array_equal(bits(img_tight), bits(ref_tight[0]))
    assert np.array_equal(bits(img_moved), bits(ref_moved[0]))


def test_update_with_frames_queued_and_after_full_uploads(native, oracle):
    """An update with four frames queued: they finish on the old geometry (the shape of test_scene_change_and_interleaved_contexts).  A full upload after updates
    behaves as ever, and after a full upload of a scene of another size the update form takes the new count."""
    from rvpt_amd import RenderSettings, scene
    W, H = 64, 48
    a, b = scene_by_name("default"), scene_by_name("showcase")
    cam = identity_camera(W / H)
    moved_a = scene.wobble(a[0], 0.9, 0.1 * extent(a[0]))
    moved_b = scene.wobble(b[0], 0.9, 0.1 * extent(b[0]))
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(a[2], a[0], a[1])
        for f in range(4):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ctx.update_triangles(moved_a)  # with 4 frames queued
        assert ctx.query() is False
        img_old = ctx.read()
        img_moved = render(ctx, cam, 3)
        ctx.upload_scene(b[2], b[0], b[1])  # a full upload of a scene of another size after an update
        img_b = render(ctx, cam, 2)
        with pytest.raises(native.NativeError, match="the uploaded scene has") as e:
            ctx.update_triangles(moved_a)  # the OLD count
        assert e.value.code == native.ERR_INVALID
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(img_b))  # ... and the scene is untouched
        ctx.update_triangles(moved_b)
        img_b_moved = render(ctx, cam, 2)
    finally:
        ctx.close()
    ref_old, _ = oracle_frames(oracle, a, cam, W, H, "bvh", [0, 1, 2, 3])
    ref_moved, _ = oracle_frames(oracle, (moved_a, a[1], scene.refit_bvh(a[2], moved_a)), cam, W, H, "bvh", [0, 1, 2])
    ref_b, _ = oracle_frames(oracle, b, cam, W, H, "bvh", [0, 1])
    ref_b_moved, _ = oracle_frames(oracle, (moved_b, b[1], scene.refit_bvh(b[2], moved_b)), cam, W, H, "bvh", [0, 1])
    assert np.array_equal(bits(img_old), bits(ref_old[3])) and np.array_equal(bits(img_moved), bits(ref_moved[2]))
    assert np.array_equal(bits(img_b), bits(ref_b[1])) and np.array_equal(bits(img_b_moved), bits(ref_b_moved[1]))


@pytest.mark.parametrize("traversal", ["bvh", "brute"])
def test_update_errors_leave_the_scene_alone(native, traversal):
    """Update before any upload, with another count, with a bad shape or dtype: the documented error, and the next render is still the old scene's."""
    import ctypes
    W, H = 64, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    ctx = native.Context(W, H, 0, 0, 1, flags_of(native, traversal))
    try:
        with pytest.raises(native.NativeError, match="before any") as e:
            ctx.update_triangles(tris)
        assert e.value.code == native.ERR_INVALID
        with pytest.raises(native.NativeError, match="before any upload_scene"):
            ctx.update_triangles(tris[:0])
        ctx.upload_scene(nodes if traversal == "bvh" else None, tris, mats)
        img = render(ctx, cam, 2)
        for bad, what in ((tris[:-1], "the uploaded scene has 143"), (tris.astype(np.float64), "float32"), (tris.reshape(-1, 8), "float32"), (tris[:0], "no triangles")):
            with pytest.raises(native.NativeError, match=what) as e:
                ctx.update_triangles(bad)
            assert e.value.code == native.ERR_INVALID
        # the C form with a non-NULL material pointer and no materials is what it always was: a full upload that no material index can satisfy
        rc = ctx._L.rvpt_hip_upload_scene(ctx._h, None, 0, tris.ctypes.data_as(ctypes.c_void_p), tris.shape[0], mats.ctypes.data_as(ctypes.c_void_p), 0)
        assert rc == native.ERR_INVALID
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
    finally:
        ctx.close()


def test_caller_layout_has_no_update_form(native, monkeypatch):
    """The laboratory knob RVPT_HIP_BVH_CALLER_LAYOUT keeps the caller's node order, which has no level ranges: the update form says so and changes nothing."""
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    W, H = 64, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(nodes, tris, mats)
        img = render(ctx, cam, 1)
        with pytest.raises(native.NativeError, match="CALLER_LAYOUT") as e:
            ctx.update_triangles(tris)
        assert e.value.code == native.ERR_UNSUPPORTED
        assert np.array_equal(bits(render(ctx, cam, 1)), bits(img))
    finally:
        ctx.close()


def test_internal_checks_build_runs_the_update(native, oracle, monkeypatch):
    """The laboratory build with RVPT_HIP_DEBUG=1 (the kernels' internal checks): an update on the small scenes reports nothing and renders the oracle's image."""
    from rvpt_amd import scene
    monkeypatch.setenv("RVPT_HIP_DEBUG", "1")
    W, H = 64, 48
    for name in ("default", "cornell"):
        (tris, mats, nodes), cam = scene_and_camera(name, W, H)
        moved = scene.wobble(tris, 1.3, 0.1 * extent(tris))
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
        try:
            ctx.upload_scene(nodes, tris, mats)
            ctx.update_triangles(moved)
            got = render(ctx, cam, 1)
            ctx.wait()
        finally:
            ctx.close()
        ref, _ = oracle_frames(oracle, (moved, mats, scene.refit_bvh(nodes, moved)), cam, W, H, "bvh", [0])
        assert np.array_equal(bits(got), bits(ref[0]))


def test_renderer_update_triangles(native, oracle):
    """RVPT.update_triangles takes the triangles in the order they were added, restarts the accumulation and refits bvh_nodes when asked."""
    from rvpt_amd import RVPT, scene
    W, H = 64, 48
    tris, mats = scene.default_scene()
    r = RVPT(W, H, device=0, traversal="bvh")
    r.add_triangles(tris)
    for m in mats:
        r.add_material(m)
    r.initialize()
    try:
        for _ in range(3):
            r.update()
            r.draw()
        built = r.bvh_nodes
        moved = scene.wobble(tris, 0.6, 0.1 * extent(tris))
        r.update_triangles(moved)
        r.update()
        assert r.render_settings.current_frame == 0
        r.draw()
        r.update()
        r.draw()
        got = r.read_frame()
        assert np.array_equal(r.sorted_triangles, moved[r.primitive_indices])
        assert r.bvh_nodes.tobytes() == scene.refit_bvh(built, r.sorted_triangles).tobytes()
        with pytest.raises(native.NativeError):
            r.update_triangles(moved[:-1])
        ref, _ = oracle_frames(oracle, (r.sorted_triangles, mats, r.bvh_nodes), r.scene_camera.get_data(), W, H, "bvh", [0, 1])
        assert np.array_equal(bits(got), bits(ref[1]))
    finally:
        r.shutdown()


def test_torch_tensor_source(native):
    """A deformation that lives in a torch tensor on the context's device never visits the host; brute-force contexts need the host array and say so."""
    import torch
    from rvpt_amd import scene
    W, H = 96, 64
    (tris, mats, nodes), cam = scene_and_camera("cornell", W, H)
    moved = scene.wobble(tris, 2.7, 0.1 * extent(tris))
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, tris, mats)
        ctx.update_triangles(moved)
        from_numpy = render(ctx, cam, 2)
        ctx.update_triangles(tris)
        dev = torch.from_numpy(moved).to("cuda:0")
        dev[:, 12:] = 77.0  # the material row of the source is not read
        ctx.update_triangles(dev)
        from_torch = render(ctx, cam, 2)
        ctx.update_triangles(torch.from_numpy(moved))  # a host tensor is a host array
        from_cpu_tensor = render(ctx, cam, 2)
        with pytest.raises(native.NativeError, match="contiguous float32"):
            ctx.update_triangles(dev.double())
    finally:
        ctx.close()
    assert np.array_equal(bits(from_numpy), bits(from_torch)) and np.array_equal(bits(from_numpy), bits(from_cpu_tensor))
    d, _ = scene_and_camera("default", W, H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
    try:
        ctx.upload_scene(None, d[0], d[1])
        img = render(ctx, cam, 1)
        with pytest.raises(native.NativeError, match="device pointer") as e:
            ctx.update_triangles(torch.from_numpy(d[0]).to("cuda:0"))
        assert e.value.code == native.ERR_INVALID
        assert np.array_equal(bits(render(ctx, cam, 1)), bits(img))
    finally:
        ctx.close()


def test_million_triangle_terrain_once(native):
    """The 1 M-triangle terrain at 1920x1080, one frame, one phase: the update route equals the upload_scene(refit_bvh(...)) route bit for bit."""
    from rvpt_amd import Camera, scene
    W, H = 1920, 1080
    tris, mats = scene.heightfield_scene()
    nodes, idx = native.build_bvh(tris)
    tris = tris[idx]
    moved = scene.wobble(tris, 1.2, 0.1 * extent(tris))
    c = Camera(W / H)
    c.translation = np.array([0.0, 2.5, -5.0])
    c.rotation = np.array([0.0, 25.0, 0.0])
    cam = c.get_data()
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH | native.COUNT_SEGMENTS)
    try:
        ctx.upload_scene(nodes, tris, mats)
        still = render(ctx, cam, 1)
        s0 = ctx.stats()
        ctx.update_triangles(moved)
        got = render(ctx, cam, 1)
        s1 = ctx.stats()
        assert ctx.launch_info()[2] == 10
    finally:
        ctx.close()
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH | native.COUNT_SEGMENTS)
    try:
        ctx.upload_scene(scene.refit_bvh(nodes, moved), moved, mats)
        want = render(ctx, cam, 1)
        s2 = ctx.stats()
    finally:
        ctx.close()
    assert not np.array_equal(bits(got), bits(still))
    assert np.array_equal(bits(got), bits(want)) and (s1[0] - s0[0], s1[1] - s0[1]) == s2
