"""Sphere sweeps on the GPU: rvpt_hip_read with RVPT_HIP_FORMAT_SPHERE_SWEEPS (Context.sweep_spheres / sweep_spheres_into) against the statement
rvpt_amd/scene.py: sphere_sweeps — the header's arithmetic applied to every triangle.  The answer is defined without a walk, so ONE statement serves every kind
of context, every builder, every update form and every tree: whole records are compared byte for byte, the in quads included, no tolerance and no record left
out.  tests/test_sweep_host.py holds the record sets to their conditions and the statement to geometry, without a GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _guarded_pose as gp
import _nearest as nq
import _scene_model as sm
import _skin
import _sweep as sw
from _util import identity_camera
from test_gpu_parity import _chain_bvh
from test_ray_query import _mirrored_chain
from test_refit import bits, extent

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    n.load()
    assert n.device_count() >= 1
    return n


def kernel_constant(name, header="rvpt_nearest.h"):
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", (ROOT / "rvpt_amd" / "csrc" / header).read_text()).group(1))


def flags_of(native, names):
    fl = 0
    for name in names.split("|"):
        fl |= getattr(native, name)
    return fl


def ask(native, flags, scene3, records, upload=None):
    ctx = native.Context(64, 36, 0, 0, 1, flags)
    try:
        if upload is not None:
            upload(ctx)
        else:
            tris, mats, nodes = scene3
            ctx.upload_scene(nodes if flags & 3 else None, tris, mats)
        return ctx.sweep_spheres_into(records.copy())
    finally:
        ctx.close()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BVH_ORDERED", "TRAVERSAL_BVH|BVH_PER_LANE", "TRAVERSAL_BRUTE"])
def test_every_record_count_on_every_context(native, default_scene, flags):
    """Every kind of context gives the statement's bytes — the tree walk and the brute-force kernel alike — for the whole set of 1 095 records and for 1, 63,
    64, 65 and 257 of them, from host arrays and from device tensors"""
    import torch
    tris, records, want, _ = sw.set_named("default")
    stored, mats, nodes = default_scene
    assert stored.tobytes() == tris.tobytes()
    fl = flags_of(native, flags)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        ctx.upload_scene(nodes if fl & 3 else None, stored, mats)
        sw.check(ctx.sweep_spheres_into(records.copy()), want, records, flags)
        for n in (1, 63, 64, 65, 257):
            at = 300 - n // 2  # a window of its own per count
            sub, sub_want = records[at:at + n], want[at:at + n]
            sw.check(ctx.sweep_spheres_into(sub.copy()), sub_want, sub, f"{flags}, {n} records")
            dev = torch.from_numpy(sub.copy().view(np.float32).reshape(-1, 12)).to("cuda:0")
            assert ctx.sweep_spheres_into(dev) is dev
            sw.check(dev.cpu().numpy().view(native.SPHERE_SWEEP_DTYPE).reshape(-1), sub_want, sub, f"{flags}, {n} device records")
    finally:
        ctx.close()


def test_device_records_the_errors_and_the_empty_scene(native, default_scene):
    """Format 10 before any upload is refused.  A torch tensor on cuda:0 is answered in place.  49 bytes, a device view 4 bytes in, the formats beside 10: INVALID,
    memory untouched.  The empty scene: every record a miss.  sweep_spheres builds its records."""
    import torch
    tris, records, want, _ = sw.set_named("default")
    stored, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        host12 = torch.from_numpy(records.copy().view(np.float32).reshape(-1, 12))
        with pytest.raises(native.NativeError, match="sweep query before any full upload_scene.*no scene to ask") as e:
            ctx.sweep_spheres_into(host12.clone())
        assert e.value.code == native.ERR_INVALID
        ctx.upload_scene(nodes, stored, mats)
        dev = host12.to("cuda:0")
        assert ctx.sweep_spheres_into(dev) is dev
        sw.check(dev.cpu().numpy().view(native.SPHERE_SWEEP_DTYPE).reshape(-1), want, records, "device records")
        flat = host12.to("cuda:0").reshape(-1)  # a view that starts 4 bytes in: device records need 16-byte alignment
        keep = flat.clone()
        with pytest.raises(native.NativeError, match="sweep records on the device need 16-byte alignment") as e:
            ctx.sweep_spheres_into(flat[1:1 + 12 * 5].reshape(5, 12))
        assert e.value.code == native.ERR_INVALID and torch.equal(flat.view(torch.int32), keep.view(torch.int32))

        def read(fmt, buf, nbytes):
            return ctx._L.rvpt_hip_read(ctx._h, fmt, buf.ctypes.data_as(ctypes.c_void_p), nbytes)

        buf = records[:2].copy()
        assert read(10, buf, 49) == native.ERR_INVALID and buf.tobytes() == records[:2].tobytes()
        assert b"sweep query: dst_bytes 49 is not a multiple of the 48 bytes of a rvpt_sphere_sweep" in ctx._L.rvpt_hip_last_error(ctx._h)
        for fmt in (7, 15, 77):  # the values beside it stay unknown
            assert read(fmt, buf, 96) == native.ERR_INVALID and b"unknown format %d" % fmt in ctx._L.rvpt_hip_last_error(ctx._h)
            assert buf.tobytes() == records[:2].tobytes()
        ctx.sweep_spheres_into(records[:3].copy())  # a successful query leaves last_error as it was
        assert b"unknown format 77" in ctx._L.rvpt_hip_last_error(ctx._h)
        assert ctx.sweep_spheres_into(records[:0].copy()).shape == (0,)
        assert ctx.sweep_spheres_into(torch.zeros((0, 12), device="cuda:0")).shape == (0, 12)
        some = np.arange(0, records.shape[0], 9)
        out = ctx.sweep_spheres(records["org"][some], records["dir"][some], records["radius"][some], records["tmax"][some])
        assert out.dtype == native.SPHERE_SWEEP_DTYPE and out.tobytes() == want[some].tobytes()
        ctx.upload_scene(None, np.zeros((0, 16), np.float32), mats)  # the empty scene answers every record with a miss
        empty = ctx.sweep_spheres_into(records.copy())
        assert (empty["prim"] == sw.NO_PRIM).all()
        sw.check(empty, sw.answer(np.zeros((0, 16), np.float32), records), records, "the empty scene")
    finally:
        ctx.close()


def test_every_builder_gives_the_same_bytes(native):
    """The default scene in the caller's order.  build_scene numbers the CALLER'S order through the stored permutation, so the three device builders return the
    same bytes — the statement's on the caller's array.  A tree made by rvpt_bvh_build and uploaded in its leaf order is numbered in that order: the statement's
    on it, and the same t for every record."""
    from rvpt_amd import scene
    tris, records, want, _ = sw.set_named("caller")
    mats = scene.default_materials()
    got = {}
    for method in ("lbvh", "ploc", "sah"):
        got[method] = ask(native, native.TRAVERSAL_BVH, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, method) == method or pytest.fail("fell back"))
        sw.check(got[method], want, records, method)
    assert got["lbvh"].tobytes() == got["ploc"].tobytes() == got["sah"].tobytes()
    nodes, order = native.build_bvh(tris)
    stored = np.ascontiguousarray(tris[order])
    host = ask(native, native.TRAVERSAL_BVH, (stored, mats, nodes), records)
    sw.check(host, sw.answer(stored, records), records, "host")
    assert host["t"].tobytes() == want["t"].tobytes()
    hit = want["prim"] != sw.NO_PRIM
    rows = np.flatnonzero(hit)  # the triangle the host tree's numbering names is the caller's winner, or one that ties with it
    named = np.asarray(order)[host["prim"][rows]]
    with np.errstate(all="ignore"):
        has, t, _, _, _ = scene.sweep_sphere_triangles(records["org"][rows], records["dir"][rows], records["radius"][rows], records["tmax"][rows], tris)
    k = np.arange(rows.size)
    assert has[k, named].all() and t[k, named].tobytes() == want["t"][rows].tobytes() and (named == want["prim"][rows]).sum() > rows.size // 2


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_stacked_duplicates_the_smaller_number_wins(native, flags):
    """The multi-hit tests' 12 layers with exact duplicates: both copies have the winning t, and the smaller reported number comes back"""
    from rvpt_amd import scene
    tris, records, want, _ = sw.set_named("layers")
    mats = scene.default_materials()
    fl = getattr(native, flags)
    if fl & 3:
        got = ask(native, fl, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, "sah"))
    else:
        got = ask(native, fl, (tris, mats, None), records)
    sw.check(got, want, records, f"layers, {flags}")


def test_a_callers_tree_with_loose_boxes(native, default_scene):
    """Boxes grown at random still contain their vertices: the walk visits more and answers the same."""
    tris, records, want, _ = sw.set_named("default")
    stored, mats, nodes = default_scene
    loose = nq.grown_boxes(nodes, 5)
    assert loose.tobytes() != np.ascontiguousarray(nodes).tobytes()
    sw.check(ask(native, native.TRAVERSAL_BVH, (stored, mats, loose), records), want, records, "loose boxes")


@pytest.mark.parametrize("shape", ["chain", "mirrored"])
def test_a_deep_chain_runs_into_the_overflow_stack(native, shape):
    """A chain of 48 leaves: the tree's height sizes the stack at 48 slots, of which kQueryLdsLevels = 8 live in LDS; a large sphere that moves along the chain
    stacks a leaf at every level in one of the two leanings"""
    from rvpt_amd import scene
    assert kernel_constant("kQueryLdsLevels", "rvpt_query.h") == 8
    tris, records, want, _ = sw.set_named("chain")
    mats = scene.default_materials()
    nodes = _chain_bvh(tris) if shape == "chain" else _mirrored_chain(tris)
    along = sw.make_records([(0, 0, -3), (0, 0, 12), (3, 3, -3), (0.1, 0, 20)], [(0, 0, 1), (0, 0, -1), (-0.2, -0.2, 1), (0, 0, -1)], [4.0, 4.0, 0.5, 0.01], [np.inf, np.inf, np.inf, 30.0])
    records = np.concatenate([records, along])
    want = np.concatenate([want, sw.answer(tris, along)])
    assert (want["prim"][-4:] != sw.NO_PRIM).sum() >= 3
    sw.check(ask(native, native.TRAVERSAL_BVH, (tris, mats, nodes), records), want, records, shape)


def test_the_37_level_ladder(native):
    """tests/_device_state.py's geometric ladder built by "sah" on the device: a tree 37 levels high, 29 of them past the LDS part of the stack, with coordinates
    from 2^75 down to 2^-60 whose products overflow and vanish.  Nothing is asserted of the geometry but the counts below: the walk ends, and the device gives the
    statement's bytes — its NaN rules included."""
    import _device_state as ds
    from rvpt_amd import scene
    tris = ds.ladder(30, 300, 1)
    assert ds.LADDERS[(30, 300, 1)]["height"] == 37 and tris.shape[0] == 330
    mats = scene.default_materials()
    xs = np.sort(ds.vertices(tris).astype(np.float64)[:, 0, 0])
    h = 2.0 ** -60
    pick = xs[::7]
    org = [(0.0, 0.0, 0.0), (0.0, h, h), (float(xs[-1]) * 4, h, h), (float(xs[150]), 1.5 * h, 1.5 * h)] + [(float(x) * 0.5, 1.25 * h, 1.25 * h) for x in pick] + \
          [(float(x) * 0.5, 1.0, 1.0) for x in pick[::4]]
    d = [(2.0 ** 80, 0.0, 0.0), (1.0, 0.0, 0.0), (-float(xs[-1]), 0.0, 0.0), (0.0, 0.0, 0.0)] + [(float(x), 0.0, 0.0) for x in pick] + [(float(x), -1.0, -1.0) for x in pick[::4]]
    r = [1.0, 2.0 ** -70, 2.0 ** 60, h] + [float(x) / 128 for x in pick] + [0.25] * len(pick[::4])
    with np.errstate(all="ignore"):
        records = sw.make_records(org, d, r, np.inf)
        want = sw.answer(tris, records)
    hits = int((want["prim"] != sw.NO_PRIM).sum())
    assert hits >= 20 and hits < records.shape[0] and len(set(want["prim"].tolist())) > 10
    got = ask(native, native.TRAVERSAL_BVH, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, "sah") == "sah" or pytest.fail("fell back"))
    sw.check(got, want, records, "ladder, sah")


@pytest.mark.parametrize("name", ["field512", "field578"])
def test_brute_force_at_the_tile_boundary(native, name):
    """Height fields of exactly kNearestTileTris = 512 triangles — one LDS tile — and of 578 — a tile and a tail — on a brute-force context, and the same bytes
    from the tree walk of a device build"""
    from rvpt_amd import scene
    tile = kernel_constant("kNearestTileTris")
    tris, records, want, _ = sw.set_named(name)
    assert tile == 512 and tris.shape[0] == int(name[5:]) and (tris.shape[0] == tile or tris.shape[0] // tile == 1)
    mats = scene.default_materials()
    past = want["prim"][want["prim"] != sw.NO_PRIM]
    assert name == "field512" or (past >= tile).sum() > 5  # winners from the tail
    sw.check(ask(native, native.TRAVERSAL_BRUTE, (tris, mats, None), records), want, records, f"brute force, {name}")
    sw.check(ask(native, native.TRAVERSAL_BVH, None, records, upload=lambda ctx: ctx.build_scene(tris, mats, "lbvh")), want, records, f"lbvh, {name}")


@pytest.mark.parametrize("form", ["plain", "sparse", "pose", "skin", "guarded pose"])
@pytest.mark.parametrize("traversal", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_sweeps_answer_for_the_mesh_as_the_last_update_left_it(native, traversal, form):
    """After update_triangles (plain, indices=), pose_parts, bind_skin + skin, and a guarded pose update that rebuilds: the statement on the rows
    tests/_scene_model.py's model holds after the same step, in the caller's order — which is also the numbering after the rebuild"""
    from rvpt_amd import scene
    tris, records, want, _ = sw.set_named("caller")
    mats = scene.default_materials()
    n = tris.shape[0]
    fl = getattr(native, traversal)
    model = sm.Model(bvh=bool(fl & 3))
    model.build("lbvh", tris)
    ctx = native.Context(64, 36, 0, 0, 1, fl)
    try:
        assert ctx.build_scene(tris, mats, "lbvh") == "lbvh"
        before = ctx.sweep_spheres_into(records.copy())
        sw.check(before, want, records, f"{form}: before")
        if form == "plain":
            moved = scene.wobble(tris, 1.9, 0.1 * extent(tris))
            model.update(moved)
            ctx.update_triangles(moved)
        elif form == "sparse":
            idx = np.random.RandomState(7).permutation(n)[:n // 3]
            rows = scene.wobble(tris, 1.9, 0.1 * extent(tris))[idx]
            model.update_sparse(idx, rows)
            ctx.update_triangles(rows, indices=idx)
        elif form == "pose":
            f, c = gp.part_of(n)
            moves = [gp.turned(tris, f, c, 25.0), gp.carried(tris, *gp.second_part_of(n))]
            model.pose(moves)
            ctx.pose_parts(moves)
        elif form == "skin":
            rec, m = _skin.weights(tris, 6), _skin.bones(tris, 6, 0.4)
            model.bind(rec)
            model.skin(m)
            ctx.bind_skin(rec)
            ctx.skin(m)
        else:
            f, c = gp.part_of(n)
            moves = [gp.turned(tris, f, c, 90.0)]
            expected = model.pose_guarded(moves, 1.02)
            report = ctx.pose_parts(moves, rebuild_above=1.02)
            if traversal == "TRAVERSAL_BRUTE":
                assert report is None and expected is None
            else:
                assert report.rebuilt and expected.rebuilt
        got = ctx.sweep_spheres_into(records.copy())
    finally:
        ctx.close()
    sw.check(got, sw.answer(model.current, records), records, form)
    assert not sw.same_bytes(got, before)


def test_the_out_quad_pipes_into_a_surface_read(native, default_scene):
    """(prim, u, v) of every hit goes into format 6 as it stands: the point and normal are scene.surface_points' on the stored rows, and the point lies at the
    radius from the centre at t, to rounding"""
    from rvpt_amd import scene
    tris, records, want, _ = sw.set_named("default")
    stored, mats, nodes = default_scene
    ctx = native.Context(64, 36, 0, 0, 1, native.TRAVERSAL_BVH)
    try:
        ctx.upload_scene(nodes, stored, mats)
        got = ctx.sweep_spheres_into(records.copy())
        surf = ctx.surface_points(got["prim"], got["u"], got["v"])
    finally:
        ctx.close()
    expect = scene.surface_points(stored, want["prim"], want["u"], want["v"])
    assert surf.tobytes() == expect.tobytes()
    hit = (want["prim"] != sw.NO_PRIM) & (want["t"] > 0) & (records["radius"] > 0.01 * sw.box_of(tris)[1])
    centre = records["org"][hit].astype(np.float64) + records["dir"][hit].astype(np.float64) * want["t"][hit].astype(np.float64)[:, None]
    gap = np.linalg.norm(centre - surf["point"][hit].astype(np.float64), axis=1) / records["radius"][hit] - 1.0
    assert hit.sum() > 300 and np.abs(gap).max() < 2.0 ** -5  # (the statement's tolerance of tests/test_sweep_host.py: these are the same numbers)
    miss = want["prim"] == sw.NO_PRIM
    assert (surf["mat"][miss] == sw.NO_PRIM).all() and not surf["point"][miss].any()


@pytest.mark.parametrize("flags", ["TRAVERSAL_BVH", "TRAVERSAL_BRUTE"])
def test_a_sweep_leaves_frames_untouched(native, default_scene, flags):
    """Two accumulated frames, a sweep, a third frame: image, stats, the timing's dispatch count, launch_info, cull_info and last_error equal a context that
    never asked."""
    from rvpt_amd import RenderSettings
    _, records, _, _ = sw.set_named("default")
    tris, mats, nodes = default_scene
    fl = getattr(native, flags) | native.COUNT_SEGMENTS | native.TIMING
    cam = identity_camera(64 / 36)
    out = []
    for asks in (False, True):
        ctx = native.Context(64, 36, 0, 0, 1, fl)
        try:
            ctx.upload_scene(nodes if fl & 3 else None, tris, mats)
            if asks:
                ctx.sweep_spheres_into(records[:300].copy())  # before any set_frame
            for f in range(3):
                ctx.set_frame(RenderSettings(max_bounces=8, aa=2, current_frame=f).pack(), cam)
                ctx.dispatch()
                if asks and f == 1:
                    ctx.sweep_spheres_into(records.copy())  # (with frames in flight: the call waits for them)
            img = ctx.read()
            out.append((bits(img).tobytes(), ctx.stats(), ctx.timing()[2], ctx.launch_info(), ctx.cull_info(), ctx._L.rvpt_hip_last_error(ctx._h)))
        finally:
            ctx.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("traversal", ["bvh", "brute"])
def test_rvpt_sweep_spheres_with_contacts_on_a_cube(native, traversal):
    """RVPT.sweep_spheres(contacts=True) over a host-built tree: spheres of radius 0.25 sent at the six faces of a cube of half side 0.75 touch at
    t = 2 - 0.75 - 0.25 = 1, the contact is the face's point under the centre and the stored normal is the face's axis; prim numbers the triangles as ADDED.  A
    sphere that starts inside the cube's surface reports t = 0, one sent away misses."""
    import _crossings as cr
    from rvpt_amd import RVPT, scene
    tris = cr.cube_scene(0.75, (0.0, 0.0, 0.0))
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    off = np.where(axes == 0, np.array([0.125, -0.25, 0.375], np.float32), np.float32(0))  # in the face's plane, on neither diagonal of the face
    org = np.concatenate([axes * 2 + off, axes * 0.75 + off, axes * 2 + off]).astype(np.float32)
    dirv = np.concatenate([-axes, np.zeros((6, 3), np.float32), axes])
    r = RVPT(64, 36, device=0, traversal=traversal)
    try:
        r.add_triangles(tris)
        for m in scene.default_materials():
            r.add_material(m)
        r.initialize()
        rec, surf = r.sweep_spheres(org, dirv, 0.25, contacts=True)
        plain = r.sweep_spheres(org, dirv, 0.25)
    finally:
        r.shutdown()
    assert plain.tobytes() == rec.tobytes() and rec.dtype == native.SPHERE_SWEEP_DTYPE and surf.dtype == native.SURFACE_POINT_DTYPE
    assert (rec["t"][:6] == 1.0).all() and (rec["t"][6:12] == 0.0).all() and (rec["prim"][:12] < tris.shape[0]).all()
    assert (rec["prim"][12:] == sw.NO_PRIM).all() and np.isinf(rec["t"][12:]).all() and (surf["mat"][12:] == sw.NO_PRIM).all()
    want_point = org[:6] - axes * 1.25  # the centre at t = 1, moved by the radius onto the face
    assert np.abs(surf["point"][:6] - want_point).max() < 1e-6
    assert np.abs(np.abs((surf["normal"][:6] * axes).sum(axis=1)) - 1.0).max() < 1e-6
    verts = sw.vertices(tris)
    for k in range(6):  # prim is the ADDED triangle: its vertices lie in the face that was hit
        assert np.abs((verts[rec["prim"][k]] * axes[k]).sum(axis=1) - 0.75).max() < 1e-6, k
    assert (surf["prim"] == rec["prim"]).all() and surf["mat"][:12].max() < 16
