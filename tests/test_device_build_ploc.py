"""The PLOC build form: Context.build_scene(tris, mats, method="ploc") (RVPT_HIP_NODES_BUILD_PLOC) makes the PLOC tree on the GPU.  As in
tests/test_device_build.py everything is bit-exact: context A, given the build, renders what a fresh context B renders given upload_scene(nodes, tris[perm],
mats) with (nodes, perm) = scene.build_ploc(tris) and what the CPU oracle renders on that tree; segment and sample counts, work-groups, LDS bytes and kernel path
are equal too; the device's topology, level table, head shift, wide nodes and wide stack need themselves are compared byte for byte in tests/test_device_state.py
(equal renders do not pin them: any valid tree over the same triangles gives the same closest hits)."""
import numpy as np
import pytest

from _util import identity_camera
from test_device_build import CASES, camera_for, native, raw_scene, rendered  # noqa: F401  (native: the module's fixture)
from test_gpu_parity import oracle_frames
from test_ploc_host import nested_triangles
from test_refit import bits, extent, flags_of, render

pytestmark = pytest.mark.gpu


def ploc(ctx, tris, mats, expect="ploc"):
    assert ctx.build_scene(tris, mats, method="ploc") == expect


@pytest.mark.parametrize("name,traversal,extra,W,H,aa,batch,frames,variant", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-aa{c[5]}{'-batch' if c[6] else ''}" for c in CASES])
def test_ploc_built_scene_equals_the_host_statement(native, oracle, name, traversal, extra, W, H, aa, batch, frames, variant):
    """Every row of test_device_build's table.  (The kernel path is compared between the two contexts, not against the table's column: that column is the
    LBVH's, and another tree of the same scene may have another wide stack need.)"""
    from rvpt_amd import scene
    tris, mats = raw_scene(name)
    cam = camera_for(name, W, H)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS | (native.BVH_PER_LANE if extra == "per_lane" else 0))
    info = {}
    nodes, perm = scene.build_ploc(tris, info=info)
    assert info["tree"] == "ploc"
    got = rendered(native, fl, W, H, cam, lambda c: ploc(c, tris, mats), frames, aa, batch)
    want = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(nodes, tris[perm], mats), frames, aa, batch)
    ref, seg = oracle_frames(oracle, (tris[perm], mats, nodes), cam, W, H, traversal, list(range(frames)), aa=aa)
    print(f"{name}: {tris.shape[0]} triangles, {len(nodes)} nodes, {info}, launch {got[2]} / {want[2]}, stats {got[1]} / {want[1]}, oracle segments {seg}")
    assert got[2] == want[2], "work-groups, LDS bytes, kernel path: device build != host statement"
    assert got[1] == want[1] and got[1][0] == seg
    assert np.array_equal(bits(got[0]), bits(want[0])), "device build != upload of build_ploc's tree"
    assert np.array_equal(bits(got[0]), bits(ref[-1])), "device build != oracle on build_ploc's tree"


def test_update_after_a_ploc_build_takes_the_callers_order(native, oracle):
    """build_scene(method="ploc"), then update_triangles(moved) in the CALLER'S order == a fresh context given refit_bvh(nodes, moved[perm]); two phases, then
    the second phase once more from a torch device tensor."""
    import torch
    from rvpt_amd import scene
    W, H = 96, 64
    tris, mats = raw_scene("cornell")
    cam = camera_for("cornell", W, H)
    nodes, perm = scene.build_ploc(tris)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ploc(ctx, tris, mats)
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
    finally:
        ctx.close()


def test_rebuilds_switch_between_the_two_trees(native, oracle):
    """LBVH -> PLOC -> LBVH on one context: each call leaves exactly the tree it names."""
    from rvpt_amd import scene
    W, H = 96, 64
    tris, mats = raw_scene("terrain64")
    cam = camera_for("terrain64", W, H)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    trees = {"lbvh": scene.build_lbvh(tris), "ploc": scene.build_ploc(tris)}
    want = {k: rendered(native, fl, W, H, cam, lambda c: c.upload_scene(t[0], tris[t[1]], mats), 2, 1, False) for k, t in trees.items()}
    assert trees["lbvh"][0].tobytes() != trees["ploc"][0].tobytes()  # two trees (the LBVH's leaves hold up to two triangles: fewer nodes)
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        for method in ("lbvh", "ploc", "lbvh", "ploc"):
            assert ctx.build_scene(tris, mats, method=method) == method
            before = ctx.stats()
            got = render(ctx, cam, 2)
            now = ctx.stats()
            assert np.array_equal(bits(got), bits(want[method][0])), method
            assert (now[0] - before[0], now[1] - before[1]) == want[method][1] and ctx.launch_info()[:3] == want[method][2], method
    finally:
        ctx.close()
    ref, seg = oracle_frames(oracle, (tris[trees["ploc"][1]], mats, trees["ploc"][0]), cam, W, H, "bvh", [0, 1])
    assert np.array_equal(bits(want["ploc"][0]), bits(ref[1])) and want["ploc"][1][0] == seg


def test_torch_device_tensor_as_the_source(native):
    import torch
    W, H = 96, 64
    tris, mats = raw_scene("cornell")
    cam = camera_for("cornell", W, H)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    from_host = rendered(native, fl, W, H, cam, lambda c: ploc(c, tris, mats), 2, 1, False)
    dev = torch.from_numpy(tris).to("cuda:0")
    from_dev = rendered(native, fl, W, H, cam, lambda c: ploc(c, dev, mats), 2, 1, False)
    assert np.array_equal(bits(from_host[0]), bits(from_dev[0])) and from_host[1:] == from_dev[1:]
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
    try:
        with pytest.raises(native.NativeError, match="host array"):
            ctx.build_scene(dev[:100].contiguous(), mats, method="ploc")
        with pytest.raises(native.NativeError, match="neither"):
            ctx.build_scene(tris, mats, method="sah")
    finally:
        ctx.close()


def test_ploc_build_with_frames_queued(native, oracle):
    """A PLOC build with four frames queued: they finish on the old scene."""
    from rvpt_amd import RenderSettings, scene
    W, H = 64, 48
    a, b = raw_scene("default"), raw_scene("showcase")
    cam = identity_camera(W / H)
    nodes_a, perm_a = scene.build_ploc(a[0])
    nodes_b, perm_b = scene.build_ploc(b[0])
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ploc(ctx, a[0], a[1])
        for f in range(4):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ploc(ctx, b[0], b[1])  # with 4 frames queued
        assert ctx.query() is False
        img_a = ctx.read()
        img_b = render(ctx, cam, 3)
    finally:
        ctx.close()
    ref_a, _ = oracle_frames(oracle, (a[0][perm_a], a[1], nodes_a), cam, W, H, "bvh", [0, 1, 2, 3])
    ref_b, _ = oracle_frames(oracle, (b[0][perm_b], b[1], nodes_b), cam, W, H, "bvh", [0, 1, 2])
    assert np.array_equal(bits(img_a), bits(ref_a[3])) and np.array_equal(bits(img_b), bits(ref_b[2]))


@pytest.mark.parametrize("source", ["host", "device"])
def test_bad_material_index_changes_nothing(native, source):
    import torch
    W, H = 64, 48
    tris, mats = raw_scene("default")
    cam = identity_camera(W / H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ploc(ctx, tris, mats)
        img = render(ctx, cam, 2)
        for row, value in ((57, float(mats.shape[0])), (31, -1.0), (90, float("nan"))):
            bad = np.roll(tris, 7, axis=0).copy()  # another scene: a call that went through would show
            bad[row, 12] = value
            bad[120, 12] = 99.0  # a later offender: the FIRST one is named
            src = torch.from_numpy(bad).to("cuda:0") if source == "device" else bad
            with pytest.raises(native.NativeError, match=rf"triangle {row}: material index") as e:
                ctx.build_scene(src, mats, method="ploc")
            assert e.value.code == native.ERR_INVALID
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
        ctx.update_triangles(tris)  # ... and the stored scene is still one the update form accepts
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
    finally:
        ctx.close()


def test_brute_force_context_ignores_the_ploc_sentinel(native):
    W, H = 64, 48
    tris, mats = raw_scene("default")
    cam = identity_camera(W / H)
    fl = native.TRAVERSAL_BRUTE | native.COUNT_SEGMENTS
    a = rendered(native, fl, W, H, cam, lambda c: c.build_scene(tris, mats, method="ploc"), 2, 2, False)
    b = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(None, tris, mats), 2, 2, False)
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[1:] == b[1:]


def test_renderer_builds_a_ploc_tree_on_the_device(native, oracle):
    """RVPT(build="device-ploc"): bvh_nodes / primitive_indices / sorted_triangles are build_ploc's; update_triangles takes the order the triangles were added in."""
    from rvpt_amd import RVPT, scene
    W, H = 64, 48
    tris, mats = scene.default_scene()
    r = RVPT(W, H, device=0, traversal="bvh", build="device-ploc")
    r.add_triangles(tris)
    for m in mats:
        r.add_material(m)
    r.initialize()
    try:
        nodes, perm = scene.build_ploc(tris)
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


def test_the_fallback_input_uploads_the_lbvh_tree(native, oracle):
    """tests/test_ploc_host.py's nested triangles: the PLOC tree is a chain higher than the bound, the call says so and the scene holds build_lbvh's tree; a
    PLOC build afterwards says "ploc" again."""
    from rvpt_amd import scene
    W, H = 64, 48
    tris = nested_triangles()
    mats = scene.default_materials()
    info = {}
    nodes, perm = scene.build_ploc(tris, info=info)
    assert info["tree"] == "lbvh" and nodes.tobytes() == scene.build_lbvh(tris)[0].tobytes()
    cam = identity_camera(W / H)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    got = rendered(native, fl, W, H, cam, lambda c: ploc(c, tris, mats, expect="lbvh"), 2, 1, False)
    want = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(nodes, tris[perm], mats), 2, 1, False)
    ref, seg = oracle_frames(oracle, (tris[perm], mats, nodes), cam, W, H, "bvh", [0, 1])
    assert got[1:] == want[1:] and got[1][0] == seg
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[0]), bits(ref[1]))
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ploc(ctx, tris, mats, expect="lbvh")
        assert b"LBVH tree" in ctx._L.rvpt_hip_last_error(ctx._h)
        ploc(ctx, *raw_scene("default"))
        assert ctx._L.rvpt_hip_last_error(ctx._h) == b""
    finally:
        ctx.close()
