"""Box queries on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_BOX_OVERLAPS / RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k) (Context.box_overlaps / box_overlaps_into)
against the statement rvpt_amd/scene.py: box_overlaps — the header's test applied to every triangle.  The answer is defined without a walk, so ONE statement
serves every kind of context, every builder, every update form and every tree: whole records and groups are compared byte for byte, the followers' poisoned
in quads included, no tolerance and no record left out."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _box as bx
import _crossings as cr
import _guarded_pose as gp
import _multi_hit as mh
import _nearest as nq
import _skin
from _util import identity_camera
from test_gpu_parity import _chain_bvh
from test_ray_query import _mirrored_chain
from test_refit import bits, extent

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KS = list(bx.KS)


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    n.load()
    assert n.device_count() >= 1
    return n


def kernel_constant(name, header="rvpt_nearest.h"):
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", (ROOT / "rvpt_amd" / "csrc" / header).read_text()).group(1))


@pytest.fixture(scope="module")
def group_sets(default_scene):
    """k -> (records, the statement's answer in stored order) on the default scene's 143 triangles: about 2 000 boxes of every kind (tests/_box.py: boxes_of;
    tests/test_box_host.py holds the set to its conditions on the CPU).  Computed once."""
    tris = default_scene[0]
    assert tris.shape[0] == 143
    sets = {k: bx.box_set(tris, 7, k) for k in KS}
    for k, (_, want) in sets.items():
        zero, listed_whole, overfull, invalid, n = bx.census(want, k)
        assert zero - invalid > 50 and listed_whole > 200 and overfull > 200 and invalid > 30 and n % 64
    return sets


def ask(native, flags, scene3, records, k, upload=None):
    ctx = native.Context(64, 36, 0, 0, 1, flags)
    try:
        if upload is not None:
            upload(ctx)
        else:
            tris, mats, nodes = scene3
            ctx.upload_scene(nodes if flags & 3 else None, tris, mats)
        return ctx.box_overlaps_into(records.copy(), k=k)
    finally:
        ctx.close()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BVH_ORDERED", "TRAVERSAL_BVH|BVH_PER_LANE", "TRAVERSAL_BRUTE"])
def test_every_k_on_every_context(native, default_scene, group_sets, flags, k):
    """Every kind of context gives the statement's bytes at every k — the tree walk and the brute-force kernel alike — for about 2 000 groups, for 45 groups
    (fewer than a wave) and for one group."""
    records, want = group_sets[k]
    fl = 0
    for name in flags.split("|"):
        fl |= getattr(native, name)
    tris, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
        got = ctx.box_overlaps_into(records.copy(), k=k)
        bx.check(got, want, records, k, f"{flags}, k = {k}")
        few, few_want = records[-45 * k:], want[-45 * k:]
        bx.check(ctx.box_overlaps_into(few.copy(), k=k), few_want, few, k, f"{flags}, k = {k}, 45 groups")
        one = int(np.flatnonzero(want.reshape(-1, k)["count"][:, 0] > bx.slots(k))[0])
        sub = records[one * k:(one + 1) * k]
        bx.check(ctx.box_overlaps_into(sub.copy(), k=k), want[one * k:(one + 1) * k], sub, k, f"{flags}, k = {k}, one group")
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_k_1_is_format_9_and_64_and_69_stay_unknown(native, default_scene, group_sets, flags):
    """FORMAT_BOX_OVERLAPS_K(1) = 65 returns format 9's bytes on the same records and speaks with format 9's messages; 64 and 69 are unknown formats and leave
    dst as it was"""
    records, want = group_sets[1]
    tris, mats, nodes = default_scene
    fl = getattr(native, flags)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if fl & 3 else None, tris, mats)

        def read(fmt, buf, nbytes):
            return ctx._L.rvpt_hip_read(ctx._h, fmt, buf.ctypes.data_as(ctypes.c_void_p), nbytes)

        by_9, by_65 = records.copy(), records.copy()
        assert read(9, by_9, by_9.nbytes) == 0 and read(65, by_65, by_65.nbytes) == 0
        assert by_9.tobytes() == by_65.tobytes() == want.tobytes()
        said = []
        for fmt in (9, 65):
            buf = records[:2].copy()
            assert read(fmt, buf, 49) == native.ERR_INVALID and buf.tobytes() == records[:2].tobytes()
            said.append(ctx._L.rvpt_hip_last_error(ctx._h))
        assert said[0] == said[1] and b"box query: dst_bytes 49 is not a multiple of the 48 bytes of a rvpt_box_overlap" in said[0] and b"k =" not in said[0]
        buf = records[:6].copy()
        for fmt in (64, 69):
            assert read(fmt, buf, 48 * 6) == native.ERR_INVALID and b"unknown format %d" % fmt in ctx._L.rvpt_hip_last_error(ctx._h)
            assert buf.tobytes() == records[:6].tobytes()
        ctx.box_overlaps_into(records[:3].copy())  # a successful query leaves last_error as it was
        assert b"unknown format 69" in ctx._L.rvpt_hip_last_error(ctx._h)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def cornell_sets():
    from rvpt_amd import scene
    tris, mats = scene.cornell_scene(2)
    assert tris.shape[0] == 2300
    tris = np.ascontiguousarray(tris[np.random.RandomState(2).permutation(tris.shape[0])])
    sets = {k: bx.box_set(tris, 17, k, n_surface=330, n_off=100, n_far=20, n_flat=30, n_invalid=12, n_paged=60) for k in (1, 3)}
    for k, (_, want) in sets.items():
        zero, listed_whole, overfull, _, n = bx.census(want, k)
        assert zero > 20 and listed_whole > 30 and overfull > 100 and n % 64
    return tris, mats, sets


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("method", ["host", "lbvh", "ploc", "sah"])
def test_every_builder_gives_the_statements_bytes(native, cornell_sets, method, k):
    """2 300 shuffled triangles.  build_scene numbers the CALLER'S order through the stored permutation, so the three device builders return the same bytes —
    the statement's on the caller's array.  A tree made by rvpt_bvh_build and uploaded in its leaf order is numbered in that order: the statement's on it."""
    tris, mats, sets = cornell_sets
    records, want = sets[k]
    if method == "host":
        nodes, order = native.build_bvh(tris)
        stored = np.ascontiguousarray(tris[order])
        got = ask(native, native.TRAVERSAL_BVH, (stored, mats, nodes), records, k)
        want = bx.answer(stored, records, k)
        assert not bx.same_bytes(want, sets[k][1])
    else:
        got = ask(native, native.TRAVERSAL_BVH, None, records, k, upload=lambda ctx: ctx.build_scene(tris, mats, method) == method or pytest.fail("fell back"))
    bx.check(got, want, records, k, f"{method}, k = {k}")


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_stacked_duplicates_count_once_each(native, flags, k):
    """The multi-hit tests' 12 layers with four exact duplicates: a box through a doubled layer counts both copies, each once"""
    from rvpt_amd import scene
    tris, zs = mh.layered_scene()
    mats = scene.default_materials()
    lo, hi, first, flg = bx.boxes_of(tris, 23, n_surface=300, n_off=60, n_far=10, n_flat=30, n_invalid=6, n_paged=30)
    records = bx.groups(lo, hi, first, flg, k)
    want = bx.answer(tris, records, k)
    doubled = sorted(set(zs[[j for j in range(len(zs)) if (zs == zs[j]).sum() == 4]].tolist()))
    thin = bx.groups([(-0.9, -0.9, z) for z in doubled], [(0.9, 0.9, z) for z in doubled], 0, 0, k)  # a plane probe in a doubled layer: its four triangles
    assert len(doubled) == 2 and bx.lists(bx.answer(tris, thin, k), k)[0].tolist() == [4, 4]
    records, want = np.concatenate([records, thin]), np.concatenate([want, bx.answer(tris, thin, k)])
    fl = getattr(native, flags)
    if fl & 3:
        got = ask(native, fl, None, records, k, upload=lambda ctx: ctx.build_scene(tris, mats, "sah"))
    else:
        got = ask(native, fl, (tris, mats, None), records, k)
    bx.check(got, want, records, k, f"layers, {flags}, k = {k}")


@pytest.mark.parametrize("k", [2, 4])
def test_a_callers_tree_with_loose_boxes(native, default_scene, group_sets, k):
    """Boxes grown at random still contain their vertices: the walk visits more and answers the same."""
    records, want = group_sets[k]
    tris, mats, nodes = default_scene
    loose = nq.grown_boxes(nodes, 5)
    assert loose.tobytes() != np.ascontiguousarray(nodes).tobytes()
    bx.check(ask(native, native.TRAVERSAL_BVH, (tris, mats, loose), records, k), want, records, k, f"loose boxes, k = {k}")


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("shape", ["chain", "mirrored"])
def test_the_overflow_stack(native, shape, k):
    """The chain of 48 leaves of the point queries' case 4: the tree's height sizes the stack at 48 slots, of which kQueryLdsLevels = 8 live in LDS; a box that
    holds the whole chain stacks a leaf at every level in one of the two leanings.  Boxes of every size along it, the whole-scene box among them."""
    from rvpt_amd import scene
    assert kernel_constant("kQueryLdsLevels", "rvpt_query.h") == 8
    rng = np.random.RandomState(11)
    quads = []
    for i in range(24):
        z, s, c = 1.0 + 0.25 * i, 0.3 + 0.05 * i, rng.uniform(-0.5, 0.5, 2)
        p = [(c[0] - s, c[1] - s, z), (c[0] + s, c[1] - s, z), (c[0] + s, c[1] + s, z), (c[0] - s, c[1] + s, z)]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    tris = scene.make_triangles(quads, 0)
    mats = scene.default_materials()
    nodes = _chain_bvh(tris) if shape == "chain" else _mirrored_chain(tris)
    lo, hi, first, flg = bx.boxes_of(tris, 3, n_surface=200, n_off=60, n_far=10, n_flat=30, n_invalid=6, n_paged=30)
    whole = bx.groups([(-5, -5, 0)] * 3, [(5, 5, 9)] * 3, [0, 17, 47], 0, k)
    records = np.concatenate([bx.groups(lo, hi, first, flg, k), whole])
    want = bx.answer(tris, records, k)
    assert bx.lists(want, k)[0][-3:].tolist() == [48, 31, 1]
    assert (bx.lists(want, k)[0] > 24).sum() > 20  # boxes that hold more than half the chain
    bx.check(ask(native, native.TRAVERSAL_BVH, (tris, mats, nodes), records, k), want, records, k, f"{shape}, k = {k}")


def test_the_37_level_ladder(native):
    """tests/_device_state.py's geometric ladder built by "sah" on the device: thirty levels that peel one triangle each, then the cluster in median splits —
    a tree 37 levels high, 29 of them past the LDS part of the stack, with coordinates from 2^75 down to 2^-60 whose products overflow and vanish.  Nothing is
    asserted of the geometry but the counts below: the walk ends, and the device gives the statement's bytes — its NaN rules included."""
    import _device_state as ds
    from rvpt_amd import scene
    k = 4
    tris = ds.ladder(30, 300, 1)
    assert ds.LADDERS[(30, 300, 1)]["height"] == 37 and tris.shape[0] == 330
    mats = scene.default_materials()
    v = ds.vertices(tris).astype(np.float64)
    xs = np.sort(v[:, 0, 0])
    lo = [(0.0, 0.0, 0.0), (float(xs[0]) / 2, 0.0, 0.0), (0.0, 0.0, 0.0)] + [(float(x) * 0.75, 0.0, 0.0) for x in xs[::7]]
    hi = [(2.0 ** 80, 1.0, 1.0), (float(xs[-1]) * 2, 2.0 ** -58, 2.0 ** -58), (float(xs[300]), 1.0, 1.0)] + [(float(x) * 1.5, 2.0 ** -59, 2.0 ** -59) for x in xs[::7]]
    with np.errstate(all="ignore"):
        records = bx.groups(lo, hi, 0, 0, k)
        want = bx.answer(tris, records, k)
    count = bx.lists(want, k)[0]
    assert count[0] == count[1] == 330 and count[2] >= 300 and (count[3:] >= 1).all() and (count[3:] < 330).any()
    got = ask(native, native.TRAVERSAL_BVH, None, records, k, upload=lambda ctx: ctx.build_scene(tris, mats, "sah") == "sah" or pytest.fail("fell back"))
    bx.check(got, want, records, k, "ladder, sah")


def test_brute_force_tiles_wrap(native):
    """Cornell + 9 k on a brute-force context: 9 164 triangles are seventeen tiles of kNearestTileTris = 512 rows and a tail; members of one box come from many
    tiles and the 15 smallest numbers from the first ones.  A few hundred boxes, and the same bytes from the tree walk of a device build."""
    from rvpt_amd import scene
    tile = kernel_constant("kNearestTileTris")
    assert tile == 512
    tris, mats = scene.cornell_scene(3)
    assert tris.shape[0] == 9164 and tris.shape[0] // tile == 17 and tris.shape[0] % tile
    k = 4
    lo, hi, first, flg = bx.boxes_of(tris, 13, n_surface=200, n_off=50, n_far=10, n_flat=20, n_invalid=6, n_paged=50)
    records = bx.groups(lo, hi, first, flg, k)
    want = bx.answer(tris, records, k)
    count, numbers = bx.lists(want, k)
    full = numbers[:, -1] != bx.NO_PRIM
    tiles = numbers[full] // tile
    assert len(set((numbers[numbers != bx.NO_PRIM] // tile).tolist())) == 18 and (tiles.min(axis=1) != tiles.max(axis=1)).sum() > 10 and count.max() > 2000
    bx.check(ask(native, native.TRAVERSAL_BRUTE, (tris, mats, None), records, k), want, records, k, "brute force, eighteen tiles")
    bx.check(ask(native, native.TRAVERSAL_BVH, None, records, k, upload=lambda ctx: ctx.build_scene(tris, mats, "lbvh")), want, records, k, "the same boxes, lbvh")


@pytest.mark.parametrize("form", ["plain", "sparse", "pose", "skin", "guarded pose"])
@pytest.mark.parametrize("traversal", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_queries_answer_for_the_mesh_as_the_last_update_left_it(native, traversal, form):
    """After update_triangles (plain, indices=), pose_parts, bind_skin + skin, and a guarded pose update that rebuilds, as in the point queries' case 6: the
    statement on the triangles the update form's own numpy statement gives, in the caller's order — which is also the numbering after the rebuild.  k = 2."""
    from rvpt_amd import scene
    k = 2
    tris, mats = scene.default_scene()
    n = tris.shape[0]
    fl = getattr(native, traversal)
    lo, hi, first, flg = bx.boxes_of(tris, 19, n_surface=500, n_off=150, n_far=20, n_flat=40, n_invalid=10, n_paged=60)
    records = bx.groups(lo, hi, first, flg, k)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        assert ctx.build_scene(tris, mats, "lbvh") == "lbvh"
        before = ctx.box_overlaps_into(records.copy(), k=k)
        bx.check(before, bx.answer(tris, records, k), records, k, f"{form}: before")
        if form == "plain":
            moved = scene.wobble(tris, 1.9, 0.1 * extent(tris))
            ctx.update_triangles(moved)
        elif form == "sparse":
            idx = np.random.RandomState(7).permutation(n)[:n // 3]
            moved = tris.copy()
            moved[idx, :12] = scene.wobble(tris, 1.9, 0.1 * extent(tris))[idx, :12]
            ctx.update_triangles(moved[idx], indices=idx)
        elif form == "pose":
            f, c = gp.part_of(n)
            moves = [gp.turned(tris, f, c, 25.0), gp.carried(tris, *gp.second_part_of(n))]
            moved = scene.pose_parts(tris, moves)
            ctx.pose_parts(moves)
        elif form == "skin":
            rec, m = _skin.weights(tris, 6), _skin.bones(tris, 6, 0.4)
            moved = scene.skin_triangles(tris, rec, m)
            ctx.bind_skin(rec)
            ctx.skin(m)
        else:
            f, c = gp.part_of(n)
            moves = [gp.turned(tris, f, c, 90.0)]
            step = gp.step(gp.built(tris, "lbvh"), moves, 1.02, "lbvh")
            assert step.rebuilt
            moved = step.state.current
            report = ctx.pose_parts(moves, rebuild_above=1.02)
            assert report is None if traversal == "TRAVERSAL_BRUTE" else report.rebuilt
        got = ctx.box_overlaps_into(records.copy(), k=k)
    finally:
        ctx.close()
    bx.check(got, bx.answer(moved, records, k), records, k, form)
    assert not bx.same_bytes(got, before)


def test_device_records_the_errors_and_the_empty_scene(native, default_scene, group_sets):
    """A torch tensor on cuda:0, in place, and a (n, k) host array: the bytes a flat host query returns.  48 * k * n + 48 bytes (the message gives k), a view 4
    bytes in, no scene: INVALID, memory untouched.  The empty scene: count 0 and 0xFFFFFFFF for every group.  box_overlaps builds its groups."""
    import torch
    k = 3
    records, want = group_sets[k]
    tris, mats, nodes = default_scene
    n = records.shape[0] // k
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        host12 = torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12))
        with pytest.raises(native.NativeError, match="box query before any full upload_scene.*no scene to ask") as e:
            ctx.box_overlaps_into(host12.clone(), k=k)
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, tris, mats)
        dev = host12.to("cuda:0")
        assert ctx.box_overlaps_into(dev, k=k) is dev
        bx.check(dev.cpu().numpy().view(native.BOX_OVERLAP_DTYPE).reshape(-1), want, records, k, "device records")
        two_d = records.copy().reshape(n, k)  # a (n, k) host array
        assert ctx.box_overlaps_into(two_d, k=k) is two_d
        bx.check(two_d, want, records, k, "a (n, k) array")
        flat = host12.to("cuda:0").reshape(-1)  # a view that starts 4 bytes in: device records need 16-byte alignment
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="box records on the device need 16-byte alignment") as e:
            ctx.box_overlaps_into(flat[1:1 + 12 * 2 * k].reshape(2 * k, 12), k=k)
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))
        buf = records[:5 * k + 1].copy()  # 48 * k * 5 + 48 bytes, through the C call
        rc = ctx._L.rvpt_hip_read(ctx._h, native.FORMAT_BOX_OVERLAPS_K(k), buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes)
        said = ctx._L.rvpt_hip_last_error(ctx._h)
        assert rc == native.ERR_INVALID and b"box query with k = 3" in said and str(buf.nbytes).encode() in said and b"multiple" in said and b"rvpt_box_overlap" in said
        assert buf.tobytes() == records[:5 * k + 1].tobytes()
        assert ctx.box_overlaps_into(records[:0].copy(), k=k).shape == (0,)
        assert ctx.box_overlaps_into(torch.zeros((0, 12), device="cuda:0"), k=k).shape == (0, 12)
        # box_overlaps builds the groups itself: zeros where the tests' records carry poison or noise, the same out quads
        g = want.reshape(n, k)
        some = np.arange(0, n, 9)
        out = ctx.box_overlaps(g["lo"][some, 0], g["hi"][some, 0], g["prim_from"][some, 0], k=k)
        assert out.shape == (some.size, k) and out.dtype == native.BOX_OVERLAP_DTYPE
        assert out.view(np.uint32).reshape(some.size, k, 12)[:, :, 8:].tobytes() == np.ascontiguousarray(g[some]).view(np.uint32).reshape(some.size, k, 12)[:, :, 8:].tobytes()
        assert not out["flags"].any() and not out["lo"][:, 1:].any()
        # prim_from above the number of triangles: nothing takes part
        high = ctx.box_overlaps(g["lo"][some, 0], g["hi"][some, 0], tris.shape[0], k=k)
        assert not bx.lists(high, k)[0].any() and (bx.lists(high, k)[1] == bx.NO_PRIM).all()
        # the empty scene answers every group with nothing
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)
        empty = ctx.box_overlaps_into(records.copy(), k=k)
        assert not bx.lists(empty, k)[0].any()
        bx.check(empty, bx.answer(np.zeros((0, 16), np.float32), records, k), records, k, "the empty scene")
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_a_query_leaves_frames_untouched(native, default_scene, group_sets, flags):
    """Two accumulated frames, a box query, a third frame: image, stats, the timing's dispatch count, launch_info, cull_info and last_error equal a context
    that never asked."""
    from rvpt_amd import RenderSettings
    k = 4
    records, _ = group_sets[k]
    tris, mats, nodes = default_scene
    fl = getattr(native, flags) | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for asks in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
            if asks:
                ctx.box_overlaps_into(records[:300 * k].copy(), k=k)  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.box_overlaps_into(records[:1000 * k].copy(), k=k)  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info(), ctx._L.rvpt_hip_last_error(ctx._h)))
        finally:
            ctx.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("traversal", ["bvh", "brute"])
def test_rvpt_overlapping_pages_to_the_whole_set(native, traversal):
    """RVPT.overlapping over a host-built tree: boxes that hold more than 40 triangles of a height field come back whole, ascending, numbered as the triangles
    were ADDED — the statement's full set on the added order; RVPT.box_overlaps renumbers every listed slot the same way and leaves the count a count."""
    from rvpt_amd import RVPT, scene
    tris, mats = scene.heightfield_scene(cells=12)  # 288 triangles
    r = RVPT(64, 36, device=0, traversal=traversal)
    try:
        r.add_triangles(tris)
        for m in mats:
            r.add_material(m)
        r.initialize()
        lo, hi, _, _ = bx.boxes_of(tris, 5, n_surface=60, n_off=20, n_far=4, n_flat=9, n_invalid=6, n_paged=0)
        with np.errstate(all="ignore"):
            valid = np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1)
            meets = scene.triangle_box_overlaps(tris, lo, hi) & valid[:, None]
        assert (meets.sum(axis=1) > 40).sum() > 10 and meets.sum(axis=1).max() == 288
        got = r.overlapping(lo, hi)
        assert len(got) == lo.shape[0]
        for i, numbers in enumerate(got):
            assert numbers.dtype == np.uint32 and numbers.tolist() == np.flatnonzero(meets[i]).tolist(), i
        rec = r.box_overlaps(lo, hi, k=2)
        count, numbers = bx.lists(rec, 2)
        assert (count == meets.sum(axis=1)).all()
        for i in range(lo.shape[0]):
            listed = numbers[i][numbers[i] != bx.NO_PRIM]
            assert listed.size == min(count[i], 7) and len(set(listed.tolist())) == listed.size and meets[i, listed].all(), i
    finally:
        r.shutdown()


@pytest.mark.parametrize("shape", ["cube", "icosphere"])
def test_rvpt_voxelize_is_the_statement_and_brackets_inside(native, shape):
    """RVPT.voxelize on an 8^3 grid: the cells the statement counts a triangle in.  The surface cells separate inside from outside: wherever RVPT.inside
    classifies the centres of two face neighbours differently, the mesh passes between the centres, hence through one of the two closed cells."""
    from rvpt_amd import RVPT, renderer, scene
    tris = cr.cube_scene(0.8, (0.05, -0.02, 0.03)) if shape == "cube" else cr.icosphere_scene(0.9, (0.04, 0.01, -0.03))
    origin, cell, dims = (-1.25, -1.25, -1.25), 2.5 / 8, (8, 8, 8)
    r = RVPT(64, 36, device=0, traversal="bvh")
    try:
        r.add_triangles(tris)
        for m in scene.default_materials():
            r.add_material(m)
        r.initialize()
        grid = r.voxelize(origin, cell, dims)
        lo, hi = renderer.voxel_boxes(origin, cell, dims)
        want = scene.triangle_box_overlaps(tris, lo, hi).any(axis=1).reshape(dims)
        assert grid.dtype == bool and grid.shape == dims and (grid == want).all()
        assert 50 < grid.sum() < 400 and not grid[0].any() and not grid[3:5, 3:5, 3:5].any()  # a shell: nothing at the rim, nothing at the heart
        inside = r.inside(((lo.astype(np.float64) + hi) / 2).astype(np.float32)).reshape(dims)
        assert inside[3:5, 3:5, 3:5].all() and not inside[0].any()
        pairs = 0
        for axis in range(3):
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[axis], b[axis] = slice(0, -1), slice(1, None)
            differ = inside[tuple(a)] != inside[tuple(b)]
            assert (grid[tuple(a)] | grid[tuple(b)])[differ].all(), axis
            pairs += int(differ.sum())
        assert pairs > 50
    finally:
        r.shutdown()
