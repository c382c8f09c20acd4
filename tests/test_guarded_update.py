"""The guarded update of rvpt_hip_upload_scene (include/rvpt_hip.h: RVPT_HIP_NODES_UPDATE_GUARDED, Context.update_triangles(rebuild_above=)): refit, the SAH cost of
the refitted tree computed on the device, and past a limit a rebuild by the builder that made the tree.  The reported numbers against scene.tree_cost on the
numpy statement of the same tree; the decision against the one numpy takes; the images, bit for bit, against a plain update (refitted) or a fresh build of the
moved triangles (rebuilt)."""
import ctypes
import math

import numpy as np
import pytest

from test_device_build import camera_for, native, rendered  # noqa: F401  (native: the module's fixture)
from test_refit import bits, extent, render

pytestmark = pytest.mark.gpu

LIMIT = 1.25
PHASE = 1.9
REL = 1e-9  # double summation over n <= 2^21 terms in any order errs by at most n * 2^-53 = 2.3e-10 relative


def scene_of(name):
    from rvpt_amd import scene
    if name == "terrain16":  # 512 triangles; the LBVH has more than 256 nodes: stage two of the cost sees more than one partial
        return scene.heightfield_scene(16)
    if name == "terrain64":  # 8192 triangles: some 33 partials and more
        return scene.heightfield_scene(64)
    if name == "cornell1":  # five materials
        return scene.cornell_scene(subdiv_levels=1)
    if name == "two":  # one node
        tris, mats = scene.default_scene()
        return tris[100:102].copy(), mats
    return scene.default_scene()


_TREES, _MOVED = {}, {}


def tree_of(name, method):
    """(tris, mats, nodes, perm) of the numpy statement of the tree build_scene(method) makes — built once, shared and left unchanged"""
    if (name, method) not in _TREES:
        from rvpt_amd import scene
        tris, mats = scene_of(name)
        tris = np.ascontiguousarray(tris)
        nodes, perm = {"lbvh": scene.build_lbvh, "ploc": scene.build_ploc, "sah": scene.build_sah}[method](tris)[:2]
        _TREES[name, method] = (tris, mats, nodes, perm)
    return _TREES[name, method]


def moved_of(name, amplitude, phase=PHASE):
    if (name, amplitude, phase) not in _MOVED:
        from rvpt_amd import scene
        tris = np.ascontiguousarray(scene_of(name)[0])
        _MOVED[name, amplitude, phase] = scene.wobble(tris, phase, amplitude * extent(tris))
    return _MOVED[name, amplitude, phase]


def numpy_costs(name, method, moved):
    """(cost of the refitted tree, base cost) by scene.tree_cost"""
    from rvpt_amd import scene
    _, _, nodes, perm = tree_of(name, method)
    return scene.tree_cost(scene.refit_bvh(nodes, moved[perm])), scene.tree_cost(nodes)


def camera_of(name, W, H):
    return camera_for({"cornell1": "cornell"}.get(name, name), W, H)


def raw_guarded(native, ctx, tris, permille, mats=None, n=None):
    """the C call itself: (return code, rvpt_hip_last_error)"""
    tris = np.ascontiguousarray(tris, dtype=np.float32)
    mp, mn = (mats.ctypes.data_as(ctypes.c_void_p), mats.shape[0]) if mats is not None else (None, 0)
    rc = ctx._L.rvpt_hip_upload_scene(ctx._h, None, native.nodes_update_guarded(permille), tris.ctypes.data_as(ctypes.c_void_p), tris.shape[0] if n is None else n, mp, mn)
    return rc, (ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode()


def close(a, b):
    return abs(a - b) <= REL * abs(b)


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_the_guarded_count_is_a_form_of_the_call(native, method):
    """until this form existed the call answered "BVH context needs nodes" """
    tris, mats, _, _ = tree_of("default", method)
    ctx = native.Context(80, 48, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        rc, said = raw_guarded(native, ctx, tris, 0)
        assert rc == 0, said
        assert said.startswith("guarded update: cost ") and said.endswith(" permille: refitted")
    finally:
        ctx.close()


NUMBER_CASES = [("terrain16", "lbvh"), ("terrain16", "ploc"), ("terrain16", "sah"), ("terrain64", "lbvh"), ("two", "lbvh")]


@pytest.mark.parametrize("name,method", NUMBER_CASES, ids=[f"{n}-{m}" for n, m in NUMBER_CASES])
def test_the_reported_cost_is_tree_cost_of_the_refitted_tree(native, name, method):
    tris, mats, nodes, perm = tree_of(name, method)
    if (name, method) == ("terrain16", "lbvh"):
        assert len(nodes) > 256
    if name == "terrain64":
        assert len(nodes) > 32 * 256
    if name == "two":
        assert len(nodes) == 1
    moved = moved_of(name, 0.1)
    want, want_base = numpy_costs(name, method, moved)
    ctx = native.Context(80, 48, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        rep = ctx.update_triangles(moved, rebuild_above=math.inf)
        said = ctx._L.rvpt_hip_last_error(ctx._h).decode()
        print(f"{name} {method}: {len(nodes)} nodes; device: {said}; numpy: cost {want!r}, base {want_base!r}")
        assert not rep.rebuilt and rep.tree is None
        assert close(rep.cost, want), (rep.cost, want)
        assert close(rep.base_cost, want_base), (rep.base_cost, want_base)
        assert rep.ratio == rep.cost / rep.base_cost
        assert f"cost {rep.cost:.17g}, base cost {rep.base_cost:.17g}, limit 0 permille: refitted" in said  # %.17g: the doubles come back as they were
        ctx.update_triangles(moved, rebuild_above=math.inf)
        assert ctx._L.rvpt_hip_last_error(ctx._h).decode() == said, "the same tree must give the same 64 bits on every run"
    finally:
        ctx.close()


DECISION_CASES = [(n, m, a) for n in ("terrain16", "default") for m in ("lbvh", "ploc", "sah") for a in (0.02, 0.3)] + \
                 [("cornell1", m, a) for m in ("lbvh", "ploc", "sah") for a in (0.02, 0.5)]  # Cornell at 0.3 lies within 5 % of the limit for PLOC (1.259): 0.5 clears it


@pytest.mark.parametrize("name,method,amplitude", DECISION_CASES, ids=[f"{n}-{m}-{a}" for n, m, a in DECISION_CASES])
def test_the_decision_and_the_image(native, name, method, amplitude):
    """limit 1.25.  Ratios in numpy (refitted / rest-pose tree), amplitude 0.02 / 0.3: terrain16 lbvh 1.027 / 1.697, ploc 1.042 / 1.916, sah 1.048 / 1.959; default
    lbvh 1.011 / 1.476, ploc 1.010 / 1.606, sah 1.007 / 1.637; Cornell (subdiv 1) at 0.02 / 0.5: lbvh 0.969 / 1.051, ploc 0.994 / 1.499, sah 1.007 / 1.605."""
    W, H = 96, 64
    tris, mats, _, _ = tree_of(name, method)
    moved = moved_of(name, amplitude)
    cost, base = numpy_costs(name, method, moved)
    ratio = cost / base
    print(f"{name} {method} amplitude {amplitude}: numpy ratio {ratio:.4f}")
    if abs(ratio / LIMIT - 1.0) < 0.05:
        pytest.fail(f"misconfigured case: the ratio {ratio:.4f} lies within 5 % of the limit {LIMIT}")
    expect_rebuild = ratio > LIMIT
    if name != "cornell1":
        assert expect_rebuild == (amplitude == 0.3)
    cam = camera_of(name, W, H)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl), native.Context(W, H, 0, 0, 1, fl)
    try:
        assert a.build_scene(tris, mats, method=method) == method
        rep = a.update_triangles(moved, rebuild_above=LIMIT)
        print(f"device: {rep}")
        assert close(rep.cost, cost) and close(rep.base_cost, base)
        assert rep.rebuilt == expect_rebuild
        got = render(a, cam, 2)
        if not expect_rebuild:
            assert rep.tree is None
            assert b.build_scene(tris, mats, method=method) == method
            assert b.update_triangles(moved) is None
            assert np.array_equal(bits(got), bits(render(b, cam, 2))), "refitted: the image of the plain update"
            return
        assert rep.tree == method
        assert b.build_scene(moved, mats, method=method) == method
        want = render(b, cam, 2)
        assert a.launch_info()[:3] == b.launch_info()[:3]
        assert np.array_equal(bits(got), bits(want)), "rebuilt: the image of a fresh build of the moved triangles (tree, mat_id rows, materials)"
        # the permutation was replaced: a plain update in the caller's order lands where it lands on the fresh context
        moved2 = moved_of(name, 0.05, 0.7)
        a.update_triangles(moved2)
        b.update_triangles(moved2)
        got2, want2 = render(a, cam, 2), render(b, cam, 2)
        assert not np.array_equal(bits(got2), bits(got))
        assert np.array_equal(bits(got2), bits(want2)), "after the rebuild the update form goes through the NEW permutation"
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("limit,amplitude", [(math.inf, 0.3), (LIMIT, 0.02), (LIMIT, 0.3)])
def test_numpy_array_and_device_tensor_report_and_render_the_same(native, limit, amplitude):
    import torch
    W, H = 80, 48
    name, method = "terrain16", "sah"
    tris, mats, _, _ = tree_of(name, method)
    moved = moved_of(name, amplitude)
    cam = camera_of(name, W, H)
    out = []
    for source in ("numpy", "torch"):
        ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
        try:
            assert ctx.build_scene(tris, mats, method=method) == method
            src = moved if source == "numpy" else torch.from_numpy(moved).to("cuda:0")
            rep = ctx.update_triangles(src, rebuild_above=limit)
            out.append((rep, ctx._L.rvpt_hip_last_error(ctx._h), bits(render(ctx, cam, 2)), ctx.launch_info()[:3]))
        finally:
            ctx.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][0].rebuilt == (limit == LIMIT and amplitude == 0.3)
    assert out[0][3] == out[1][3] and np.array_equal(out[0][2], out[1][2])


def test_bad_arguments_leave_the_scene_alone(native):
    W, H = 80, 48
    tris, mats, _, _ = tree_of("default", "sah")
    moved = moved_of("default", 0.3)
    cam = camera_of("default", W, H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        rc, said = raw_guarded(native, ctx, tris, 0)
        assert rc == native.ERR_INVALID and "before any full upload_scene" in said  # the update form's own words
        assert ctx.build_scene(tris, mats, method="sah") == "sah"
        img = bits(render(ctx, cam, 2))
        for permille in (999, 65536, 1, 0xFFFFF):
            rc, said = raw_guarded(native, ctx, moved, permille)
            assert rc == native.ERR_INVALID and "1000 .. 65535" in said, (permille, said)
        rc, said = raw_guarded(native, ctx, moved, 1250, mats=mats)
        assert rc == native.ERR_INVALID and "no materials" in said
        rc, said = raw_guarded(native, ctx, moved, 0, mats=mats)
        assert rc == native.ERR_INVALID and "no materials" in said
        rc, said = raw_guarded(native, ctx, moved[:-1], 1250)
        assert rc == native.ERR_INVALID and "the uploaded scene has 143" in said
        for bad in (0.5, 0.9994, 65.6, -1.0, float("nan"), -math.inf):
            with pytest.raises(native.NativeError, match="rebuild_above"):
                ctx.update_triangles(moved, rebuild_above=bad)
        assert np.array_equal(bits(render(ctx, cam, 2)), img)
        # the band's ends are forms of the call
        for permille in (1000, 65535):
            rc, said = raw_guarded(native, ctx, tris, permille)
            assert rc == 0 and f"limit {permille} permille: " in said, said
    finally:
        ctx.close()


def test_after_an_ordinary_upload_there_is_no_builder_to_name(native):
    from rvpt_amd import scene
    W, H = 80, 48
    tris, mats, nodes, perm = tree_of("default", "sah")
    moved = moved_of("default", 0.3)
    cam = camera_of("default", W, H)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes, tris[perm], mats)
        img = bits(render(ctx, cam, 2))
        with pytest.raises(native.NativeError, match="no builder") as e:
            ctx.update_triangles(moved[perm], rebuild_above=LIMIT)
        assert e.value.code == native.ERR_INVALID
        assert np.array_equal(bits(render(ctx, cam, 2)), img)
        rep = ctx.update_triangles(moved[perm], rebuild_above=math.inf)  # the leaf order of the upload, as the update form takes it there
        cost, base = numpy_costs("default", "sah", moved)
        assert not rep.rebuilt and close(rep.cost, cost) and close(rep.base_cost, base)
        refit = scene.refit_bvh(nodes, moved[perm])
        want = rendered(native, fl, W, H, cam, lambda c: c.upload_scene(refit, moved[perm], mats), 2, 1, False)
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(want[0]))
    finally:
        ctx.close()


def test_brute_force_contexts_take_the_plain_update(native):
    W, H = 80, 48
    tris, mats = scene_of("default")
    moved = moved_of("default", 0.3)
    cam = camera_of("default", W, H)
    a, b = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE), native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BRUTE)
    try:
        a.upload_scene(None, tris, mats)
        b.upload_scene(None, tris, mats)
        rc, said = raw_guarded(native, a, moved, 1250)
        assert rc == 0 and said == ""
        assert a.update_triangles(moved, rebuild_above=LIMIT) is None
        b.update_triangles(moved)
        assert np.array_equal(bits(render(a, cam, 2)), bits(render(b, cam, 2)))
    finally:
        a.close()
        b.close()


def test_the_base_cost_after_a_rebuild_is_the_new_trees(native):
    name, method = "terrain16", "ploc"
    tris, mats, _, _ = tree_of(name, method)
    moved = moved_of(name, 0.3)
    ctx = native.Context(80, 48, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        assert ctx.build_scene(tris, mats, method=method) == method
        first = ctx.update_triangles(moved, rebuild_above=LIMIT)
        said = ctx._L.rvpt_hip_last_error(ctx._h).decode()
        assert first.rebuilt and first.tree == "ploc"
        new_base = float(said.rsplit("new base cost ", 1)[1])
        from rvpt_amd import scene
        assert close(new_base, scene.tree_cost(scene.build_ploc(moved)[0]))
        again = ctx.update_triangles(moved, rebuild_above=LIMIT)
        assert not again.rebuilt and again.base_cost == new_base
        assert abs(again.ratio - 1.0) <= REL
        # and the build forms report as they always did: nothing after a SAH build
        assert ctx.build_scene(tris, mats, method="sah") == "sah"
        assert ctx._L.rvpt_hip_last_error(ctx._h) == b""
    finally:
        ctx.close()


def test_renderer_keyword_and_its_host_statement(native):
    """RVPT(build="device-sah").update_triangles(moved, rebuild_above=): after a rebuild bvh_nodes is the statement of a fresh build from the moved triangles"""
    from rvpt_amd import RVPT, scene
    tris, mats = scene_of("terrain16")
    moved_small, moved_large = moved_of("terrain16", 0.02), moved_of("terrain16", 0.3)
    r = RVPT(80, 48, device=0, traversal="bvh", build="device-sah")
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        assert r.update_triangles(moved_small) is None
        rep = r.update_triangles(moved_small, rebuild_above=LIMIT)
        assert not rep.rebuilt
        assert np.array_equal(r.bvh_nodes, scene.refit_bvh(scene.build_sah(np.ascontiguousarray(tris))[0], moved_small[r.primitive_indices]))
        rep = r.update_triangles(moved_large, rebuild_above=LIMIT)
        assert rep.rebuilt and rep.tree == "sah"
        nodes, perm = scene.build_sah(moved_large)[:2]
        assert np.array_equal(r.bvh_nodes, nodes) and np.array_equal(r.primitive_indices, perm)
        assert np.array_equal(r.sorted_triangles, moved_large[perm])
    finally:
        r.shutdown()
