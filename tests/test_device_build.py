"""The device BVH build: the build form of rvpt_hip_upload_scene (Context.build_scene) makes the tree on the GPU from triangles in the caller's order.
Everything here is bit-exact: context A, given build_scene(tris, mats), renders what a fresh context B renders given upload_scene(nodes, tris[perm], mats) with
(nodes, perm) = scene.build_lbvh(tris) — the same tree stated in numpy — and what the CPU oracle renders on that tree; work-groups, LDS bytes and kernel path
of the launch are equal too.  That agrees with the host's level table, head shift, wide nodes and wide stack need but does not pin them, nor the topology: a
walk finds the same closest hit in any valid tree over the same triangles.  tests/test_device_state.py reads the device's tree back and compares the bytes."""
import numpy as np
import pytest

from _util import identity_camera
from test_gpu_parity import oracle_frames
from test_refit import bits, extent, flags_of, render

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def raw_scene(name):
    """(tris in the order the scene's generator makes them, mats)"""
    from rvpt_amd import scene
    if name == "terrain64":
        return scene.heightfield_scene(64)
    if name == "terrain1m":
        return scene.heightfield_scene()
    if name == "one":
        tris, mats = scene.default_scene()
        return tris[100:101].copy(), mats
    if name == "n_le_L":
        tris, mats = scene.default_scene()
        return tris[100:100 + scene.LBVH_LEAF_TRIS].copy(), mats
    if name == "identical300":
        tris, mats = scene.default_scene()
        tris = np.repeat(tris[100:101], 300, axis=0)
        tris[:, 12] = np.arange(300) % mats.shape[0]  # the caller's order shows in the material rows
        return tris, mats
    return {"default": scene.default_scene, "cornell": scene.cornell_scene, "showcase": scene.materials_showcase_scene}[name]()


def camera_for(name, W, H):
    from rvpt_amd import Camera
    c = Camera(W / H)
    if name == "cornell":
        c.translation = np.array([0.0, 2.0, -1.9])
    elif name.startswith("terrain"):
        c.translation = np.array([0.0, 2.5, -5.0])
        c.rotation = np.array([0.0, 25.0, 0.0])
    else:
        return identity_camera(W / H)
    return c.get_data()


def rendered(native, fl, W, H, cam, upload, frames, aa, batch):
    """(image, (segments, samples), launch_info()[:3]) of a fresh context after upload(ctx)"""
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        upload(ctx)
        img = render(ctx, cam, frames, aa=aa, batch=batch)
        return img, ctx.stats(), ctx.launch_info()[:3]
    finally:
        ctx.close()


CASES = [
    # scene, traversal, extra flag, W, H, aa, batched, frames, kernel path
    ("default", "bvh", 0, 96, 64, 1, False, 2, 11),       # the LDS-resident wide walk
    ("cornell", "bvh", 0, 96, 64, 1, False, 2, 10),       # the HBM-resident 4-wide walk
    ("terrain64", "bvh", 0, 96, 64, 1, False, 2, 10),
    ("cornell", "bvh_ordered", 0, 80, 48, 1, False, 2, 2),  # nearer child first, binary nodes
    ("cornell", "bvh", "per_lane", 80, 48, 1, False, 2, 2),
    ("default", "bvh", "per_lane", 80, 48, 1, False, 2, 3),
    ("default", "bvh", 0, 80, 48, 2, False, 2, 11),       # aa 2
    ("cornell", "bvh", 0, 80, 48, 1, True, 2, 10),        # one launch of two frames
    ("one", "bvh", 0, 80, 48, 1, False, 2, None),         # the root is a leaf: no wide form
    ("n_le_L", "bvh", 0, 80, 48, 1, False, 2, None),
    ("identical300", "bvh", 0, 80, 48, 1, False, 2, None),  # equal codes: the index bits split
    ("terrain1m", "bvh", 0, 1920, 1080, 1, False, 1, 10),  # the 1 M-triangle terrain at 1080p, one frame
]


@pytest.mark.parametrize("name,traversal,extra,W,H,aa,batch,frames,variant", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-aa{c[5]}{'-batch' if c[6] else ''}" for c in CASES])
def test_device_built_scene_equals_the_host_statement(native, oracle, name, traversal, extra, W, H, aa, batch, frames, variant):
    from rvpt_amd import scene
    tris, mats = raw_scene(name)
    cam = camera_for(name, W, H)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS | (native.BVH_PER_LANE if extra == "per_lane" else 0))
    nodes, perm = scene.build_lbvh(tris)
    got = rendered(native, fl, W, H, cam, lambda c: c.build_scene(tris, mats), frames, aa, batch)
    want = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(nodes, tris[perm], mats), frames, aa, batch)
    ref, seg = oracle_frames(oracle, (tris[perm], mats, nodes), cam, W, H, traversal, list(range(frames)), aa=aa)
    print(f"{name}: {tris.shape[0]} triangles, {len(nodes)} nodes, launch {got[2]} / {want[2]}, stats {got[1]} / {want[1]}, oracle segments {seg}")
    if variant is not None:
        assert want[2][2] == variant
    assert got[2] == want[2], "work-groups, LDS bytes, kernel path: device build != host statement"
    assert got[1] == want[1] and got[1][0] == seg
    assert np.array_equal(bits(got[0]), bits(want[0])), "device build != upload of build_lbvh's tree"
    assert np.array_equal(bits(got[0]), bits(ref[-1])), "device build != oracle on build_lbvh's tree"


def test_update_after_a_build_takes_the_callers_order(native, oracle):
    """build_scene, then update_triangles(moved) in the CALLER'S order == a fresh context given refit_bvh(nodes, moved[perm]); two phases, then the second phase
    once more from a torch device tensor (whose material row is not read)."""
    import torch
    from rvpt_amd import scene
    W, H = 96, 64
    tris, mats = raw_scene("cornell")
    cam = camera_for("cornell", W, H)
    nodes, perm = scene.build_lbvh(tris)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.build_scene(tris, mats)
        still = render(ctx, cam, 2)
        info = ctx.launch_info()[:3]
        moved = None
        for phase in (0.7, 1.9, "torch"):
            if phase == "torch":
                ctx.update_triangles(tris)
                dev = torch.from_numpy(moved).to("cuda:0")
                dev[:, 12:] = 77.0
                ctx.update_triangles(dev)
            else:
                moved = scene.wobble(tris, phase, 0.1 * extent(tris))
                ctx.update_triangles(moved)
            got = render(ctx, cam, 2)
            assert ctx.launch_info()[:3] == info
            refit = scene.refit_bvh(nodes, moved[perm])
            want = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(refit, moved[perm], mats), 2, 1, False)
            ref, _ = oracle_frames(oracle, (moved[perm], mats, refit), cam, W, H, "bvh", [0, 1])
            assert not np.array_equal(bits(got), bits(still)), f"phase {phase}: the geometry did not move"
            assert np.array_equal(bits(got), bits(want[0])), f"phase {phase}: update after build != fresh upload of the refit tree"
            assert np.array_equal(bits(got), bits(ref[1])), f"phase {phase}: update after build != oracle"
        # an ordinary full upload afterwards: the update form takes the leaf order of that upload again
        ctx.upload_scene(nodes, tris[perm], mats)
        ctx.update_triangles(moved[perm])
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(got))
    finally:
        ctx.close()


def test_rebuild_on_moved_triangles(native, oracle):
    """A second build-form call is a rebuild: the tree of the moved triangles (another topology, another permutation), not a refit of the first."""
    from rvpt_amd import scene
    W, H = 96, 64
    tris, mats = raw_scene("terrain64")
    cam = camera_for("terrain64", W, H)
    moved = scene.wobble(tris, 1.3, 0.1 * extent(tris))
    nodes, perm = scene.build_lbvh(moved)
    assert not np.array_equal(perm, scene.build_lbvh(tris)[1])
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.build_scene(tris, mats)
        render(ctx, cam, 1)
        seen = ctx.stats()
        ctx.build_scene(moved, mats)
        got = render(ctx, cam, 2)
        now, launch = ctx.stats(), ctx.launch_info()[:3]
    finally:
        ctx.close()
    want = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(nodes, moved[perm], mats), 2, 1, False)
    ref, seg = oracle_frames(oracle, (moved[perm], mats, nodes), cam, W, H, "bvh", [0, 1])
    assert np.array_equal(bits(got), bits(want[0])) and np.array_equal(bits(got), bits(ref[1]))
    assert (now[0] - seen[0], now[1] - seen[1]) == want[1] and want[1][0] == seg and launch == want[2]


def test_torch_device_tensor_as_the_source(native):
    """A build from a torch tensor on the context's device equals the build from the host array it was copied from; brute-force contexts say they need the host."""
    import torch
    W, H = 96, 64
    tris, mats = raw_scene("cornell")
    cam = camera_for("cornell", W, H)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    from_host = rendered(native, fl, W, H, cam, lambda c: c.build_scene(tris, mats), 2, 1, False)
    dev = torch.from_numpy(tris).to("cuda:0")
    from_dev = rendered(native, fl, W, H, cam, lambda c: c.build_scene(dev, mats), 2, 1, False)
    from_cpu_tensor = rendered(native, fl, W, H, cam, lambda c: c.build_scene(torch.from_numpy(tris), mats), 2, 1, False)
    assert np.array_equal(bits(from_host[0]), bits(from_dev[0])) and from_host[1:] == from_dev[1:]
    assert np.array_equal(bits(from_host[0]), bits(from_cpu_tensor[0]))
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
    try:
        with pytest.raises(native.NativeError, match="host array"):
            ctx.build_scene(dev[:100].contiguous(), mats)
        with pytest.raises(native.NativeError, match="contiguous float32"):
            ctx.build_scene(dev.double(), mats)
    finally:
        ctx.close()


def test_build_with_frames_queued(native, oracle):
    """A build with four frames queued: they finish on the old scene (the shape of test_gpu_parity.py's scene-swap test)."""
    from rvpt_amd import RenderSettings, scene
    W, H = 64, 48
    a, _ = raw_scene("default"), None
    b = raw_scene("showcase")
    cam = identity_camera(W / H)
    nodes_a, perm_a = scene.build_lbvh(a[0])
    nodes_b, perm_b = scene.build_lbvh(b[0])
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.build_scene(a[0], a[1])
        for f in range(4):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ctx.build_scene(b[0], b[1])  # with 4 frames queued
        assert ctx.query() is False
        img_a = ctx.read()
        img_b = render(ctx, cam, 3)
    finally:
        ctx.close()
    ref_a, _ = oracle_frames(oracle, (a[0][perm_a], a[1], nodes_a), cam, W, H, "bvh", [0, 1, 2, 3])
    ref_b, _ = oracle_frames(oracle, (b[0][perm_b], b[1], nodes_b), cam, W, H, "bvh", [0, 1, 2])
    assert np.array_equal(bits(img_a), bits(ref_a[3])) and np.array_equal(bits(img_b), bits(ref_b[2]))


@pytest.mark.parametrize("source", ["host", "device"])
def test_bad_material_index_names_the_triangle_and_changes_nothing(native, source):
    """ERR_INVALID naming the first offending triangle, from a host and from a device source; the context still renders the old scene's bits."""
    import torch
    W, H = 64, 48
    tris, mats = raw_scene("default")
    cam = identity_camera(W / H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.build_scene(tris, mats)
        img = render(ctx, cam, 2)
        for row, value in ((57, float(mats.shape[0])), (31, -1.0), (90, float("nan"))):
            bad = np.roll(tris, 7, axis=0).copy()  # another scene: a call that went through would show
            bad[row, 12] = value
            bad[120, 12] = 99.0  # a later offender: the FIRST one is named
            src = torch.from_numpy(bad).to("cuda:0") if source == "device" else bad
            with pytest.raises(native.NativeError, match=rf"triangle {row}: material index") as e:
                ctx.build_scene(src, mats)
            assert e.value.code == native.ERR_INVALID
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
        ctx.update_triangles(tris)  # ... and the stored scene is still one the update form accepts
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
    finally:
        ctx.close()


def test_brute_force_context_ignores_the_sentinel(native):
    """A brute-force context ignores nodes and n_nodes as it always has: given the build form it renders what it renders given None."""
    W, H = 64, 48
    tris, mats = raw_scene("default")
    cam = identity_camera(W / H)
    fl = native.TRAVERSAL_BRUTE | native.COUNT_SEGMENTS
    a = rendered(native, fl, W, H, cam, lambda c: c.build_scene(tris, mats), 2, 2, False)
    b = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(None, tris, mats), 2, 2, False)
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[1:] == b[1:]


def test_empty_scene_and_the_pinned_error(native):
    """n_tris == 0 with the sentinel is the empty scene; no nodes and a count of 0 on a BVH context is still the "needs nodes" error."""
    import ctypes
    W, H = 64, 48
    tris, mats = raw_scene("default")
    cam = identity_camera(W / H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.build_scene(tris[:0], mats)
        sky = render(ctx, cam, 1)
        ctx.upload_scene(None, tris[:0], mats)
        assert np.array_equal(bits(render(ctx, cam, 1)), bits(sky))
        rc = ctx._L.rvpt_hip_upload_scene(ctx._h, None, 0, tris.ctypes.data_as(ctypes.c_void_p), tris.shape[0], mats.ctypes.data_as(ctypes.c_void_p), mats.shape[0])
        assert rc == native.ERR_INVALID and b"needs nodes" in ctx._L.rvpt_hip_last_error(ctx._h)
    finally:
        ctx.close()


def test_renderer_builds_on_the_device(native, oracle):
    """RVPT(build="device"): initialize() hands the triangles over as they were added; bvh_nodes / sorted_triangles are build_lbvh's (made when asked for), and
    update_triangles takes the order the triangles were added in."""
    from rvpt_amd import RVPT, scene
    W, H = 64, 48
    tris, mats = scene.default_scene()
    r = RVPT(W, H, device=0, traversal="bvh", build="device")
    r.add_triangles(tris)
    for m in mats:
        r.add_material(m)
    r.initialize()
    try:
        nodes, perm = scene.build_lbvh(tris)
        assert np.array_equal(r.primitive_indices, perm) and r.bvh_nodes.tobytes() == nodes.tobytes()
        for _ in range(2):
            r.update()
            r.draw()
        got = r.read_frame()
        ref, _ = oracle_frames(oracle, (tris[perm], mats, nodes), r.scene_camera.get_data(), W, H, "bvh", [0, 1])
        assert np.array_equal(bits(got), bits(ref[1]))
        moved = scene.wobble(tris, 0.6, 0.1 * extent(tris))
        r.update_triangles(moved)
        for _ in range(2):
            r.update()
            r.draw()
        got = r.read_frame()
        assert np.array_equal(r.sorted_triangles, moved[perm])
        assert r.bvh_nodes.tobytes() == scene.refit_bvh(nodes, moved[perm]).tobytes()
        ref, _ = oracle_frames(oracle, (moved[perm], mats, r.bvh_nodes), r.scene_camera.get_data(), W, H, "bvh", [0, 1])
        assert np.array_equal(bits(got), bits(ref[1]))
    finally:
        r.shutdown()
