"""The sparse geometry update on the GPU: rvpt_hip_upload_scene's RVPT_HIP_NODES_UPDATE_SPARSE form (Context.update_triangles(indices=)) moves the listed
triangles and refits only the paths above them.  Everything here is bit-exact: after an update the context renders what a fresh context given
upload_scene(refit_bvh(nodes, patched), patched, mats) renders — for a caller's loose tree, refit_bvh(..., touched=) — and what the CPU oracle renders there."""
import ctypes

import numpy as np
import pytest

from _util import identity_camera, scene_by_name
from test_gpu_parity import _chain_bvh, _loosen_boxes, oracle_frames
from test_refit import DEFORM, _two_leaf_tree, bits, extent, flags_of, render, scene_and_camera

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load()
    assert n.device_count() >= 1
    return n


def displaced(tris, idx, phase):
    """`tris` with the triangles idx displaced by scene.wobble at a tenth of the extent"""
    from rvpt_amd import scene
    out = tris.copy()
    out[idx, :12] = scene.wobble(tris, phase, 0.1 * extent(tris))[idx, :12]
    return out


def by_view_angle(centres, cam):
    """indices of `centres` ordered by the angle to the camera's axis, smallest first (camera data: column-major matrix, +z forward, origin in column 3)"""
    d = np.asarray(centres, dtype=np.float64) - np.asarray(cam[12:15], dtype=np.float64)
    cos = d @ np.asarray(cam[8:11], dtype=np.float64) / np.maximum(np.linalg.norm(d, axis=1), 1e-30)
    return np.argsort(-cos, kind="stable")


def leaf_runs(nodes, cam):
    """the triangle runs of the leaves, those nearest the camera's axis first: each a run inside one leaf"""
    from rvpt_amd import native as nat
    rec = np.ascontiguousarray(nodes).view(nat.NODE_DTYPE).reshape(-1)
    leaves = np.flatnonzero(rec["count"] > 0)
    b = rec["bounds"][leaves].astype(np.float64)
    leaves = leaves[by_view_angle((b[:, 0::2] + b[:, 1::2]) / 2, cam)]
    leaves = np.concatenate([leaves[rec["count"][leaves] > 1], leaves[rec["count"][leaves] == 1]])  # a run of several triangles where the tree has one
    return [np.arange(rec["first"][l], rec["first"][l] + rec["count"][l], dtype=np.int64) for l in leaves]


def single_triangles(tris, cam):
    return [np.array([t]) for t in by_view_angle(tris.reshape(-1, 4, 4)[:, :3, :3].mean(axis=1), cam)]


def first_visible(oracle, candidates, scene3, cam, W, H, traversal, phase, aa=1):
    """the first of `candidates` (index lists) whose displacement changes the oracle's two frames of the scene: a list the camera sees"""
    tris, mats, nodes = scene3
    from rvpt_amd import scene
    still, _ = oracle_frames(oracle, scene3, cam, W, H, traversal, [0, 1], aa=aa)
    for idx in candidates[:16]:
        patched = displaced(tris, idx, phase)
        img, _ = oracle_frames(oracle, (patched, mats, scene.refit_bvh(nodes, patched)), cam, W, H, traversal, [0, 1], aa=aa)
        if not np.array_equal(bits(img[1]), bits(still[1])):
            return idx
    raise AssertionError("none of the 16 candidates nearest the camera axis is seen")


def two_lists(n):
    rng = np.random.RandomState(7)
    return [np.arange(3, n, 7), rng.permutation(n)[:n // 3]]


def fresh_render(native, fl, W, H, nodes, tris, mats, cam, frames=2, aa=1, batch=False):
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes, tris, mats)
        img = render(ctx, cam, frames, aa=aa, batch=batch)
        return img, ctx.stats(), ctx.launch_info(), ctx.cull_info()
    finally:
        ctx.close()


def to_device(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to("cuda:0")


@pytest.mark.parametrize("name,traversal,extra,W,H,aa,batch,variant", DEFORM)
def test_three_sparse_updates_render_as_fresh_uploads_of_the_refit_tree(native, oracle, name, traversal, extra, W, H, aa, batch, variant):
    """ONE context, three sparse updates in a row — a run inside one leaf, every seventh triangle, a shuffled third; after each, two frames equal (a) a fresh
    context given the numpy refit of the tree over the patched triangles and (b) the oracle on that tree, counts, kernel path and LDS bytes included, and differ
    from the frames before the update."""
    from rvpt_amd import scene
    (tris, mats, nodes), cam = scene_and_camera(name, W, H)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS | (native.BVH_PER_LANE if extra == "per_lane" else 0))
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes, tris, mats)
        before = render(ctx, cam, 2, aa=aa, batch=batch)
        info = ctx.launch_info()
        assert info[2] == variant
        seen = ctx.stats()
        patched, current = tris, nodes
        in_one_leaf = first_visible(oracle, leaf_runs(nodes, cam), (tris, mats, nodes), cam, W, H, traversal, 0.7, aa=aa)
        for phase, idx in zip((0.7, 1.9, 3.4), [in_one_leaf] + two_lists(tris.shape[0])):
            patched = displaced(patched, idx, phase)
            refit = scene.refit_bvh(nodes, patched)
            assert refit.tobytes() == scene.refit_bvh(current, patched, touched=idx).tobytes()  # (a tight tree: the sparse refit is the full one)
            current = refit
            ctx.update_triangles(patched[idx], indices=idx)
            got = render(ctx, cam, 2, aa=aa, batch=batch)
            now = ctx.stats()
            assert ctx.launch_info()[1:3] == info[1:3]
            want, want_stats, want_info, _ = fresh_render(native, fl, W, H, refit, patched, mats, cam, aa=aa, batch=batch)
            ref, seg = oracle_frames(oracle, (patched, mats, refit), cam, W, H, traversal, [0, 1], aa=aa)
            assert not np.array_equal(bits(got), bits(before)), f"{idx.size} indices: the geometry did not move"
            assert np.array_equal(bits(got), bits(want)), f"{idx.size} indices: sparse update != fresh upload of the refit tree"
            assert np.array_equal(bits(got), bits(ref[1])), f"{idx.size} indices: sparse update != oracle"
            assert (now[0] - seen[0], now[1] - seen[1]) == want_stats and want_stats[0] == seg
            assert want_info[1:3] == info[1:3]
            seen, before = now, got
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["all_shuffled", "first", "last"])
def test_full_and_single_index_lists(native, which):
    """A shuffled list of every index is the plain update; a list of one entry, the first triangle and the last."""
    from rvpt_amd import scene
    W, H = 96, 64
    (tris, mats, nodes), cam = scene_and_camera("cornell", W, H)
    n = tris.shape[0]
    idx = {"all_shuffled": np.random.RandomState(3).permutation(n), "first": np.array([0]), "last": np.array([n - 1])}[which]
    patched = displaced(tris, idx, 2.1)
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl), native.Context(W, H, 0, 0, 1, fl)
    try:
        a.upload_scene(nodes, tris, mats)
        b.upload_scene(nodes, tris, mats)
        a.update_triangles(patched[idx], indices=idx.astype(np.int32 if which == "first" else np.uint64))
        b.update_triangles(patched)
        got, want = render(a, cam, 2), render(b, cam, 2)
        assert np.array_equal(bits(got), bits(want)) and a.stats() == b.stats() and a.launch_info()[1:3] == b.launch_info()[1:3]
    finally:
        a.close()
        b.close()
    want2 = fresh_render(native, fl, W, H, scene.refit_bvh(nodes, patched, touched=idx), patched, mats, cam)[0]
    assert np.array_equal(bits(got), bits(want2))


@pytest.mark.parametrize("shape", ["one_triangle", "chain", "leaves_of_72", "loose"])
@pytest.mark.parametrize("traversal", ["bvh", "bvh_ordered"])
def test_special_trees(native, oracle, shape, traversal):
    """A scene of one triangle (the root is the leaf, no wide form), the 64-level chain touched at its deepest leaf, leaves of 71 and 72 triangles, and a caller's
    tree with loose boxes: the boxes off the touched paths STAY loose — the image is that of refit_bvh(loose, patched, touched=), not of the tight tree."""
    from rvpt_amd import scene
    W, H = 80, 48
    (tris, mats, nodes), cam = scene_and_camera("cornell" if shape == "loose" else "default", W, H)
    if shape == "one_triangle":
        tris = tris[first_visible(oracle, single_triangles(tris, cam), (tris, mats, nodes), cam, W, H, traversal, 2.2, aa=2)].copy()
        nodes = np.zeros(1, dtype=native.NODE_DTYPE)
        nodes[0] = (0, 1, [0] * 6)
        nodes = scene.refit_bvh(nodes, tris)
        idx = np.array([0])
    elif shape == "chain":
        tris = tris[:64].copy()
        nodes = _chain_bvh(tris)
        idx = np.array([63])
    elif shape == "leaves_of_72":
        nodes = scene.refit_bvh(_two_leaf_tree(tris), tris)
        idx = np.arange(tris.shape[0] // 2 + 5, tris.shape[0], 3)
    else:
        nodes = _loosen_boxes(nodes, 5)
        idx = np.arange(3, tris.shape[0], 7)
    patched = displaced(tris, idx, 2.2)
    refit = scene.refit_bvh(nodes, patched, touched=idx)
    fl = flags_of(native, traversal, native.COUNT_SEGMENTS)
    ctx = native.Context(W, H, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes, tris, mats)
        render(ctx, cam, 1)
        seen = ctx.stats()
        ctx.update_triangles(patched[idx], indices=idx)
        got = render(ctx, cam, 2, aa=2)
        now = ctx.stats()
    finally:
        ctx.close()
    want, want_stats, _, _ = fresh_render(native, fl, W, H, refit, patched, mats, cam, aa=2)
    assert np.array_equal(bits(got), bits(want)) and (now[0] - seen[0], now[1] - seen[1]) == want_stats
    ref, seg = oracle_frames(oracle, (patched, mats, refit), cam, W, H, traversal, [0, 1], aa=2)
    assert np.array_equal(bits(got), bits(ref[1])) and now[0] - seen[0] == seg
    if shape == "loose":  # the case means something: the tight tree renders another image
        tight, _ = oracle_frames(oracle, (patched, mats, scene.refit_bvh(nodes, patched)), cam, W, H, traversal, [0, 1], aa=2)
        assert not np.array_equal(bits(tight[1]), bits(ref[1]))


@pytest.mark.parametrize("method", ["lbvh", "ploc", "sah"])
def test_after_build_scene_indices_are_in_the_callers_order(native, method):
    """After a build form the list numbers the triangles as the caller passed them: equal to a second context built the same way and given the plain update."""
    W, H = 96, 64
    (sorted_tris, mats, _), cam = scene_and_camera("cornell", W, H)
    rng = np.random.RandomState(17)
    tris = sorted_tris[rng.permutation(sorted_tris.shape[0])]  # the caller's order: any order
    n = tris.shape[0]
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl), native.Context(W, H, 0, 0, 1, fl)
    try:
        assert a.build_scene(tris, mats, method=method) == b.build_scene(tris, mats, method=method)
        still = render(a, cam, 2)
        render(b, cam, 2)
        patched = tris
        for phase, idx in ((0.9, np.arange(3, n, 7)), (2.6, rng.permutation(n)[:n // 3])):
            patched = displaced(patched, idx, phase)
            a.update_triangles(patched[idx], indices=idx)
            b.update_triangles(patched)
            got, want = render(a, cam, 2), render(b, cam, 2)
            assert not np.array_equal(bits(got), bits(still))
            assert np.array_equal(bits(got), bits(want)) and a.stats() == b.stats() and a.launch_info()[1:3] == b.launch_info()[1:3]
        # a rebuild replaces the permutation: the inverse the library kept must not survive it
        again = patched[rng.permutation(n)]
        a.build_scene(again, mats, method=method)
        b.build_scene(again, mats, method=method)
        idx = np.arange(1, n, 5)
        final = displaced(again, idx, 0.4)
        a.update_triangles(final[idx], indices=idx)
        b.update_triangles(final)
        assert np.array_equal(bits(render(a, cam, 2)), bits(render(b, cam, 2)))
    finally:
        a.close()
        b.close()


def test_torch_sources(native):
    """Indices and triangles both in tensors on the context's device never visit the host (the source's material rows are not read); a mixed pair and a wrong
    index dtype are refused and change nothing."""
    import torch
    W, H = 96, 64
    (tris, mats, nodes), cam = scene_and_camera("cornell", W, H)
    idx = np.random.RandomState(23).permutation(tris.shape[0])[:tris.shape[0] // 3]
    patched = displaced(tris, idx, 2.7)
    a, b = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH), native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        a.upload_scene(nodes, tris, mats)
        b.upload_scene(nodes, tris, mats)
        still = render(a, cam, 2)
        rows, where = to_device(patched[idx]), to_device(idx, torch.int32)
        for bad_idx, bad_rows, what in ((idx, rows, "mixed pair"), (where, patched[idx], "mixed pair"), (where.long(), rows, "torch.int32"), (where.float(), rows, "torch.int32")):
            with pytest.raises(native.NativeError, match=what) as e:
                a.update_triangles(bad_rows, indices=bad_idx)
            assert e.value.code == native.ERR_INVALID
        # the C seam says the same of a mixed pair
        host_idx = np.ascontiguousarray(idx, dtype=np.uint32)
        rc = a._L.rvpt_hip_upload_scene(a._h, host_idx.ctypes.data_as(ctypes.c_void_p), native.NODES_UPDATE_SPARSE, ctypes.c_void_p(rows.data_ptr()), idx.size, None, 0)
        assert rc == native.ERR_INVALID and b"both on the host or both" in a._L.rvpt_hip_last_error(a._h)
        assert np.array_equal(bits(render(a, cam, 2)), bits(still))
        rows[:, 12:] = 77.0  # garbage in the source's material rows
        a.update_triangles(rows, indices=where)
        b.update_triangles(patched[idx], indices=idx)
        got, want = render(a, cam, 2), render(b, cam, 2)
        assert not np.array_equal(bits(got), bits(still)) and np.array_equal(bits(got), bits(want))
        a.update_triangles(torch.from_numpy(tris[idx].copy()), indices=torch.from_numpy(idx.astype(np.int32)))  # host tensors are host arrays
        assert np.array_equal(bits(render(a, cam, 2)), bits(still))
    finally:
        a.close()
        b.close()


def test_frames_queued_before_the_update_finish_on_the_old_geometry(native, oracle):
    from rvpt_amd import RenderSettings, scene
    W, H = 80, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    idx = np.arange(3, tris.shape[0], 7)
    patched = displaced(tris, idx, 0.9)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, tris, mats)
        for f in range(4):
            ctx.set_frame(RenderSettings(current_frame=f).pack(), cam)
            ctx.dispatch()
        ctx.update_triangles(patched[idx], indices=idx)  # with four frames queued
        assert ctx.query() is False
        img_old = ctx.read()
        img_new = render(ctx, cam, 2)
    finally:
        ctx.close()
    ref_old, _ = oracle_frames(oracle, (tris, mats, nodes), cam, W, H, "bvh", [0, 1, 2, 3])
    ref_new, _ = oracle_frames(oracle, (patched, mats, scene.refit_bvh(nodes, patched)), cam, W, H, "bvh", [0, 1])
    assert np.array_equal(bits(img_old), bits(ref_old[3])) and np.array_equal(bits(img_new), bits(ref_new[1]))


def _raw_sparse(native, ctx, idx, rows, mats=None, device=False):
    """the C call itself (materials cannot be passed through the wrapper): (return code, message)"""
    keep = (to_device(idx.astype(np.int32)), to_device(rows)) if device else (np.ascontiguousarray(idx, dtype=np.uint32), np.ascontiguousarray(rows, dtype=np.float32))
    ptr = (lambda t: ctypes.c_void_p(t.data_ptr())) if device else (lambda a: a.ctypes.data_as(ctypes.c_void_p))
    m = None if mats is None else np.ascontiguousarray(mats, dtype=np.float32)
    rc = ctx._L.rvpt_hip_upload_scene(ctx._h, ptr(keep[0]), native.NODES_UPDATE_SPARSE, ptr(keep[1]), rows.shape[0], None if m is None else m.ctypes.data_as(ctypes.c_void_p),
                                      0 if m is None else m.shape[0])
    return rc, (ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode()


@pytest.mark.parametrize("source", ["host", "device"])
def test_errors_leave_the_scene_untouched(native, source):
    """Before any upload, more triangles than the scene has, an index out of range (its smallest list position and its value are named), an index twice (the
    smallest such value is named), materials passed: RVPT_HIP_ERR_INVALID with the same words from host and from device sources, and the same render afterwards."""
    import torch
    W, H = 80, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    n = tris.shape[0]
    device = source == "device"

    def send(ctx, idx, rows):
        idx = np.asarray(idx)
        if device:
            return ctx.update_triangles(to_device(rows), indices=to_device(idx, torch.int32))
        return ctx.update_triangles(rows, indices=idx)

    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        with pytest.raises(native.NativeError, match="before any") as e:
            send(ctx, np.arange(4), tris[:4])
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        img = render(ctx, cam, 2)
        many = np.concatenate([tris, tris[:1]])
        out_of_range = np.array([5, n + 3, 9, n, 2])       # positions 1 and 3 offend: position 1, value n + 3
        twice = np.array([40, 9, 17, 40, 9, 3, 17, 100])   # 9, 17 and 40 occur twice: 9
        cases = [(np.arange(n + 1), many, f"sparse update with {n + 1} triangles, the uploaded scene has {n}"),
                 (out_of_range, tris[:5], rf"indices\[1\] = {n + 3} is outside the {n} stored"),
                 (twice, tris[:8], "index 9 occurs more than once"),
                 (np.array([0, 1, 0xFFFFFFFF - 2 ** 32 if device else 0xFFFFFFFF]), tris[:3], r"indices\[2\] = 4294967295 is outside")]
        for idx, rows, what in cases:
            with pytest.raises(native.NativeError, match=what) as e:
                send(ctx, idx, rows)
            assert e.value.code == native.ERR_INVALID
            assert np.array_equal(bits(render(ctx, cam, 2)), bits(img)), what
        rc, msg = _raw_sparse(native, ctx, np.arange(4), tris[:4], mats=mats, device=device)
        assert rc == native.ERR_INVALID and "takes no materials" in msg
        rc, msg = _raw_sparse(native, ctx, np.arange(4), tris[:4], device=device)
        assert rc == 0, msg  # (the same call without them is the update)
        ctx.update_triangles(tris[:4], indices=np.arange(4))
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
        # a NULL list
        host_rows = np.ascontiguousarray(tris[:4])
        rc = ctx._L.rvpt_hip_upload_scene(ctx._h, None, native.NODES_UPDATE_SPARSE, host_rows.ctypes.data_as(ctypes.c_void_p), 4, None, 0)
        assert rc == native.ERR_INVALID and b"without indices" in ctx._L.rvpt_hip_last_error(ctx._h)
        assert np.array_equal(bits(render(ctx, cam, 2)), bits(img))
    finally:
        ctx.close()


def test_brute_force_context(native):
    """Brute-force contexts derive scale, table and boxes from the whole vertex set: a sparse update equals the plain update of the patched scene — image, counts,
    every cull of the packet kernel — and a device tensor is refused in the plain form's words."""
    W, H = 160, 96
    (tris, mats, _), cam = scene_and_camera("default", W, H)
    idx = np.random.RandomState(29).permutation(tris.shape[0])[:tris.shape[0] // 3]
    patched = displaced(tris, idx, 1.4)
    a, b = native.Context(W, H, 0, 0, 1, native.COUNT_SEGMENTS), native.Context(W, H, 0, 0, 1, native.COUNT_SEGMENTS)
    try:
        a.upload_scene(None, tris, mats)
        b.upload_scene(None, tris, mats)
        still = render(a, cam, 2, aa=2)
        render(b, cam, 2, aa=2)
        a.update_triangles(patched[idx], indices=idx)
        b.update_triangles(patched)
        got, want = render(a, cam, 2, aa=2), render(b, cam, 2, aa=2)
        assert not np.array_equal(bits(got), bits(still))
        assert np.array_equal(bits(got), bits(want)) and a.stats() == b.stats()
        assert a.launch_info()[2] == 6 and a.cull_info() == b.cull_info() and a.cull_info() & 0x57 == 0x57
        import torch
        with pytest.raises(native.NativeError, match="device pointer") as e:
            a.update_triangles(to_device(patched[idx]), indices=to_device(idx, torch.int32))
        assert e.value.code == native.ERR_INVALID
        with pytest.raises(native.NativeError, match="occurs more than once"):
            a.update_triangles(patched[[3, 3]], indices=np.array([3, 3]))
        assert np.array_equal(bits(render(a, cam, 2, aa=2)), bits(got))
    finally:
        a.close()
        b.close()


def test_caller_layout_has_no_sparse_form(native, monkeypatch):
    monkeypatch.setenv("RVPT_HIP_BVH_CALLER_LAYOUT", "1")
    W, H = 80, 48
    (tris, mats, nodes), cam = scene_and_camera("default", W, H)
    ctx = native.Context(W, H, 0, 0, 1, native.TRAVERSAL_BVH, lab=True)
    try:
        ctx.upload_scene(nodes, tris, mats)
        img = render(ctx, cam, 1)
        with pytest.raises(native.NativeError, match="CALLER_LAYOUT") as e:
            ctx.update_triangles(tris[:2], indices=np.array([0, 1]))
        assert e.value.code == native.ERR_UNSUPPORTED
        assert np.array_equal(bits(render(ctx, cam, 1)), bits(img))
    finally:
        ctx.close()


def test_twenty_thousand_scattered_indices(native):
    """heightfield_scene(182), 66 248 triangles, 20 000 scattered indices from the host and again from the device: thousands of threads race to flag the upper
    levels of the tree.  One 160 x 96 frame against a second context given the plain update."""
    import torch
    from rvpt_amd import Camera, scene
    W, H = 160, 96
    tris, mats = scene.heightfield_scene(182)
    nodes, order = native.build_bvh(tris)
    tris = tris[order]
    rng = np.random.RandomState(31)
    c = Camera(W / H)
    c.translation = np.array([0.0, 2.5, -5.0])
    c.rotation = np.array([0.0, 25.0, 0.0])
    cam = c.get_data()
    fl = native.TRAVERSAL_BVH | native.COUNT_SEGMENTS
    a, b = native.Context(W, H, 0, 0, 1, fl), native.Context(W, H, 0, 0, 1, fl)
    try:
        a.upload_scene(nodes, tris, mats)
        b.upload_scene(nodes, tris, mats)
        before = render(a, cam, 1)
        render(b, cam, 1)
        patched = tris
        for phase, device in ((1.2, False), (2.9, True)):
            idx = rng.permutation(tris.shape[0])[:20000]
            patched = displaced(patched, idx, phase)
            if device:
                a.update_triangles(to_device(patched[idx]), indices=to_device(idx, torch.int32))
            else:
                a.update_triangles(patched[idx], indices=idx)
            b.update_triangles(patched)
            got, want = render(a, cam, 1), render(b, cam, 1)
            assert not np.array_equal(bits(got), bits(before))
            assert np.array_equal(bits(got), bits(want)) and a.stats() == b.stats() and a.launch_info()[1:3] == b.launch_info()[1:3]
            before = got
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("build", ["host", "device-sah"])
def test_renderer_mirror(native, build):
    """RVPT.update_triangles(indices=) numbers the triangles in the order they were ADDED: the frame equals that of the full-array call on a second object, the
    mirror's host copies follow, and bvh_nodes is the sparse refit of the tree as built."""
    from rvpt_amd import RVPT, scene
    W, H = 80, 48
    tris, mats = scene.default_scene()
    idx = np.random.RandomState(37).permutation(tris.shape[0])[:tris.shape[0] // 3]
    patched = displaced(tris, idx, 0.6)
    pair = []
    for _ in range(2):
        r = RVPT(W, H, device=0, traversal="bvh", build=build)
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        pair.append(r)
    a, b = pair
    try:
        built, order = a.bvh_nodes.copy(), np.asarray(a.primitive_indices).astype(np.int64)
        for r in pair:
            for _ in range(2):
                r.update()
                r.draw()
        still = a.read_frame()
        assert a.update_triangles(patched[idx], indices=idx) is None
        b.update_triangles(patched)
        for r in pair:
            r.update()
            assert r.render_settings.current_frame == 0
            r.draw()
            r.update()
            r.draw()
        got, want = a.read_frame(), b.read_frame()
        assert not np.array_equal(bits(got), bits(still)) and np.array_equal(bits(got), bits(want))
        assert np.array_equal(np.concatenate(a.triangles), patched) and np.array_equal(a.sorted_triangles, patched[order])
        inverse = np.empty_like(order)
        inverse[order] = np.arange(order.size)
        assert a.bvh_nodes.tobytes() == scene.refit_bvh(built, patched[order], touched=inverse[idx]).tobytes() == b.bvh_nodes.tobytes()
        with pytest.raises(native.NativeError, match="do not combine"):
            a.update_triangles(patched[idx], rebuild_above=2.0, indices=idx)
    finally:
        a.shutdown()
        b.shutdown()
