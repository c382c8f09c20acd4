"""The state a BVH context holds on the device, read back (Context.scene_state, the laboratory build's rvpt_hip_selftest_scene_state) and compared byte for byte
with the numpy statements: scene.build_lbvh / build_ploc / build_sah for the build forms, scene.refit_bvh(..., touched=) for the plain and the sparse update,
scene.tree_cost for the base cost, tests/_device_state.py for the device layout, the level table, the head shift, the wide form and the sparse update's maps.

A BVH walk returns the same closest hit for any valid tree over the same triangles, so the render comparisons of test_device_build*.py, test_refit.py,
test_sparse_update.py and test_guarded_update.py cannot see a loose box, another split or tie-break, or a wrong word in a map the chosen lists do not exercise.
Nothing here renders; there are no tolerances — the two comparisons that are not of bytes are base_cost at test_guarded_update.REL and, for non-finite
vertices only, "NaN in the same places".  Finite inputs hold no zero coordinate (asserted): min / max is then independent of the order of evaluation."""
import contextlib

import numpy as np
import pytest

import _device_state as ds
from test_gpu_parity import _chain_bvh, _loosen_boxes
from test_guarded_update import REL
from test_ploc_host import nested_triangles
from test_refit import _two_leaf_tree

gpu = pytest.mark.gpu

METHODS = ("lbvh", "ploc", "sah")
# the code's own thresholds: a root leaf and kLbvhLeafTris; one wave; kTreeCostBlock; kPlocTailClusters; kSahLargeNode / kSahChunk, 4099: a work-group meets two large nodes
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4099)
BIG = 40000  # a SAH root that spans about 20 chunks
BIG_CASES = [("sah", "soup"), ("sah", "lattice"), ("lbvh", "soup"), ("lbvh", "lattice"), ("ploc", "soup")]
HOST_SIZES = (1, 2, 3, 64, 257, 1025, 2049)  # the CPU test of the layout identity


@pytest.fixture(scope="module")
def native():
    from rvpt_amd import build, native as n
    build.build_native()
    build.build_native_debug()
    n.load_lab()
    assert n.device_count() >= 1
    return n


@contextlib.contextmanager
def lab_context(native, lab=True):
    ctx = native.Context(64, 48, 0, 0, 1, native.TRAVERSAL_BVH, lab=lab)
    try:
        yield ctx
    finally:
        ctx.close()


def materials():
    from rvpt_amd import scene
    return scene.default_materials()


_TREES = {}


def numpy_tree(method, tris):
    """(nodes, perm, the tree the call reports, the builder's info or None) of the numpy statement of build_scene(method)"""
    from rvpt_amd import scene
    if method == "ploc":
        info = {}
        nodes, perm = scene.build_ploc(tris, info=info)
        return nodes, perm, info["tree"], info
    if method == "sah":
        nodes, perm, info = scene.build_sah(tris)
        return nodes, perm, method, info
    nodes, perm = scene.build_lbvh(tris)
    return nodes, perm, method, None


def tree_of(method, kind, n, info=False):
    """(tris, nodes, perm, reported tree, ds.Expected) — built once, shared and left unchanged; info=True: the builder's info as a sixth"""
    key = (method, kind, n)
    if key not in _TREES:
        tris = ds.SOUPS[kind](n, 1000 + n)
        assert ds.no_zero_coordinate(tris)
        nodes, perm, tree, built = numpy_tree(method, tris)
        _TREES[key] = (tris, nodes, perm, tree, ds.Expected(nodes, breadth_first=True), built)
    return _TREES[key] if info else _TREES[key][:5]


def cost_close(got, want):
    if np.isnan(want) or np.isinf(want):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(got - want) <= REL * abs(want)


def same_wide(got, want):
    """wide nodes of non-finite inputs: the six quads of bounds with NaN in the same places, heads and padding byte for byte"""
    return got.shape == want.shape and ds.same_floats_nan_in_place(got[:, :6, :], want[:, :6, :]) and ds.same_bytes(got[:, 6:, :].view(np.uint32), want[:, 6:, :].view(np.uint32))


def check_tree_state(state, exp, what, nan=False):
    """the pieces that follow from the tree: nodes, level table, height, head shift, wide form and its map"""
    same_f = ds.same_floats_nan_in_place if nan else ds.same_bytes
    assert state["n_nodes"] == exp.n_nodes and state["n_tris"] == exp.n_tris, what
    assert ds.same_nodes(state["nodes"], exp.nodes, nan), (what, "d_nodes", ds.first_difference(state["nodes"], exp.nodes))
    assert ds.same_bytes(state["refit_levels"], exp.levels), (what, "level table", state["refit_levels"], exp.levels)
    assert state["bvh_height"] == exp.height and state["bvh_head_shift"] == exp.head_shift, (what, state["bvh_height"], exp.height, state["bvh_head_shift"], exp.head_shift)
    assert state["n_wide"] == exp.wide.shape[0] and state["wide_stack_levels"] == exp.wide_stack_levels, (what, state["n_wide"], exp.wide.shape[0], state["wide_stack_levels"], exp.wide_stack_levels)
    heads_got, heads_want = state["wide"][:, 6:, :].view(np.uint32), exp.wide[:, 6:, :].view(np.uint32)
    assert ds.same_bytes(heads_got, heads_want), (what, "d_wide heads and padding", ds.first_difference(heads_got, heads_want))
    assert same_f(state["wide"][:, :6, :], exp.wide[:, :6, :]), (what, "d_wide boxes", ds.first_difference(state["wide"], exp.wide))
    ds.check_wide_map(state, what)


def check_build_state(state, tris, nodes, perm, exp, method, what, nan=False):
    from rvpt_amd import scene
    check_tree_state(state, exp, what, nan)
    assert state["built_by"] == method and state["have_perm"] and state["have_cost"] and not state["have_sparse_maps"] and not state["have_inv_perm"], what
    assert ds.same_bytes(state["perm"], perm), (what, "d_perm", ds.first_difference(state["perm"], perm))
    assert ds.same_bytes(state["tris"], tris[perm]), (what, "d_tris", ds.first_difference(state["tris"], tris[perm]))
    with np.errstate(all="ignore"):
        want = scene.tree_cost(nodes)
    print(f"{what}: base_cost device {state['base_cost']!r} numpy {want!r}")
    assert cost_close(state["base_cost"], want), (what, state["base_cost"], want)
    for name in ("sparse_parent", "sparse_leaf_of", "sparse_dirty", "inv_perm"):
        assert state[name].size == 0, (what, name)


def same_state(a, b, but=()):
    """every field and piece of two states, byte for byte"""
    assert a.keys() == b.keys()
    for k in a:
        if k in but:
            continue
        if isinstance(a[k], np.ndarray):
            assert ds.same_bytes(a[k], b[k]), (k, ds.first_difference(a[k], b[k]))
        elif isinstance(a[k], float):
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a[k], b[k])
        else:
            assert a[k] == b[k], (k, a[k], b[k])


# ---- CPU: the helpers themselves ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", sorted(ds.SOUPS))
@pytest.mark.parametrize("method", METHODS)
def test_the_built_trees_are_breadth_first_so_the_device_layout_is_a_shift(method, kind):
    """upload_scene's FIFO relayout of a numpy builder's tree is "every index after the root plus one", and the level table is the builder's levels"""
    for n in HOST_SIZES:
        tris, nodes, perm, _, exp = tree_of(method, kind, n)
        fifo, levels = ds.device_layout(nodes)
        assert ds.same_bytes(fifo, ds.shifted_layout(nodes)) and ds.same_bytes(fifo, exp.nodes), (method, kind, n)
        assert ds.same_bytes(levels, exp.levels) and int(levels[-1, 1]) == (1 if len(nodes) == 1 else len(nodes) + 1)
        assert sorted(perm.tolist()) == list(range(n))


def test_the_fifo_layout_of_a_tree_that_is_not_breadth_first():
    """the host builder's depth-first tree and a chain: children adjacent on even indices, parents before children, levels contiguous, the boxes carried over"""
    from rvpt_amd import native as nat, scene
    tris = ds.soup(257, 5)
    nodes, idx = nat.build_bvh(tris)
    for src in (nodes, _chain_bvh(tris[idx][:64])):
        src = np.ascontiguousarray(src).view(ds.NODE).reshape(-1)
        dev, levels = ds.device_layout(src)
        assert dev.shape[0] == src.shape[0] + 1 and dev[1].tobytes() == bytes(32)
        assert ds.same_bytes(levels, ds.levels_of(dev))
        assert tuple(levels[0]) == (0, 1) and (len(levels) == 1 or levels[1, 0] == 2) and np.array_equal(levels[2:, 0], levels[1:-1, 1])
        inner = np.flatnonzero(dev["count"] == 0)
        inner = inner[inner != 1]
        assert (dev["first"][inner] % 2 == 0).all() and (dev["first"][inner] > inner).all()
        # the same tree: walk both from the root
        stack = [(0, 0)]
        while stack:
            a, b = stack.pop()
            assert src[a]["count"] == dev[b]["count"] and src[a]["bounds"].tobytes() == dev[b]["bounds"].tobytes()
            if src[a]["count"] == 0:
                stack += [(int(src[a]["first"]), int(dev[b]["first"])), (int(src[a]["first"]) + 1, int(dev[b]["first"]) + 1)]
            else:
                assert src[a]["first"] == dev[b]["first"]
    assert scene.refit_bvh(nodes, tris[idx]).tobytes() == nodes.tobytes()


def test_the_inputs_hold_no_zero_and_the_unshifted_lattice_would():
    for kind in sorted(ds.SOUPS):
        for n in (65, 4099):
            assert ds.no_zero_coordinate(ds.SOUPS[kind](n, 1000 + n))
    t = ds.lattice(4099, 5099)
    v = ds.vertices(t) - np.float32(0.25)
    assert (v == 0).any()
    nf, pick = ds.with_non_finite(ds.soup(1025, 1), 3)
    assert pick.size >= 20 and not np.isfinite(ds.vertices(nf)[pick]).all(axis=(1, 2)).any() and ds.no_zero_coordinate(nf)
    assert np.isnan(ds.vertices(nf)).any() and np.isposinf(ds.vertices(nf)).any() and np.isneginf(ds.vertices(nf)).any()


# ---- GPU: the export itself --------------------------------------------------------------------------------------------------------------------------------

@gpu
def test_the_export_is_the_laboratorys_reports_sizes_and_changes_nothing(native):
    import ctypes as C
    tris, nodes, perm, _, exp = tree_of("lbvh", "soup", 257)
    with lab_context(native, lab=False) as rel:
        rel.build_scene(tris, materials())
        with pytest.raises(native.NativeError, match="laboratory") as e:
            rel.scene_state()
        assert e.value.code == native.ERR_UNSUPPORTED and not hasattr(rel._L, "rvpt_hip_selftest_scene_state")
    with lab_context(native) as ctx:
        with pytest.raises(native.NativeError, match="no scene") as e:
            ctx.scene_state()
        assert e.value.code == native.ERR_INVALID
        ctx.build_scene(tris, materials())
        a = ctx.scene_state()
        same_state(a, ctx.scene_state())  # twice: the same bytes
        size = C.c_size_t(0)
        buf = np.full(100 * 8, 0xA5A5A5A5, dtype=np.uint32)  # room for 100 nodes: too short
        rc = ctx._L.rvpt_hip_selftest_scene_state(ctx._h, None, native.SCENE_STATE_PIECES["nodes"][0], buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(size))
        assert rc == native.ERR_SIZE and size.value == exp.n_nodes * 32 and (buf == 0xA5A5A5A5).all()
        assert f"needs {exp.n_nodes * 32} bytes" in ctx._L.rvpt_hip_last_error(ctx._h).decode()
        assert ctx._L.rvpt_hip_selftest_scene_state(ctx._h, None, 99, None, 0, C.byref(size)) == native.ERR_INVALID
        same_state(a, ctx.scene_state())
        assert a["nodes"].nbytes == exp.n_nodes * 32 and a["tris"].nbytes == 257 * 64 and a["perm"].nbytes == 257 * 4 and a["wide"].nbytes == a["n_wide"] * 128
        assert a["wide_map"].nbytes == a["n_wide"] * 16 and a["refit_levels"].nbytes == a["bvh_height"] * 8


# ---- GPU (a): the build forms ------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", sorted(ds.SOUPS))
@pytest.mark.parametrize("method", METHODS)
def test_build_form_state_is_the_numpy_statements(native, method, kind, n):
    tris, nodes, perm, tree, exp = tree_of(method, kind, n)
    with lab_context(native) as ctx:
        assert ctx.build_scene(tris, materials(), method=method) == tree
        check_build_state(ctx.scene_state(), tris, nodes, perm, exp, method, f"{method} {kind} {n}")


@gpu
@pytest.mark.parametrize("method,kind", BIG_CASES, ids=[f"{m}-{k}" for m, k in BIG_CASES])
def test_build_form_state_at_forty_thousand(native, method, kind):
    from rvpt_amd import scene
    tris, nodes, perm, tree, exp, info = tree_of(method, kind, BIG, info=True)
    if (method, kind) == ("sah", "lattice"):
        print(f"sah lattice {BIG}: {info}")
        assert info["median_splits"] > 0 and info["max_leaf"] == 8  # what the lattice is for
    with lab_context(native) as ctx:
        assert ctx.build_scene(tris, materials(), method=method) == tree
        check_build_state(ctx.scene_state(), tris, nodes, perm, exp, method, f"{method} {kind} {BIG}")


@gpu
@pytest.mark.parametrize("n", (1025, 4099))
@pytest.mark.parametrize("kind", sorted(ds.SOUPS))
@pytest.mark.parametrize("method", METHODS)
def test_build_form_state_from_a_device_tensor(native, method, kind, n):
    import torch
    tris, nodes, perm, tree, exp = tree_of(method, kind, n)
    with lab_context(native) as ctx:
        assert ctx.build_scene(torch.from_numpy(tris).to("cuda:0"), materials(), method=method) == tree
        check_build_state(ctx.scene_state(), tris, nodes, perm, exp, method, f"{method} {kind} {n} from a tensor")


@gpu
def test_the_ploc_fallback_input_holds_the_lbvh_state(native):
    """tests/test_ploc_host.py's nested triangles (one vertex coordinate is +0, none is -0: min / max still cannot meet zeros of two signs)"""
    tris = nested_triangles()
    v = ds.vertices(tris)
    assert not (np.signbit(v) & (v == 0)).any()
    nodes, perm, tree = numpy_tree("ploc", tris)[:3]
    assert tree == "lbvh"
    exp = ds.Expected(nodes, breadth_first=True)
    with lab_context(native) as a, lab_context(native) as b:
        assert a.build_scene(tris, materials(), method="ploc") == "lbvh"
        assert b.build_scene(tris, materials(), method="lbvh") == "lbvh"
        sa, sb = a.scene_state(), b.scene_state()
        check_build_state(sa, tris, nodes, perm, exp, "ploc", "the fallback input")  # (a PLOC build that fell back is rebuilt as PLOC: built_by says so)
        same_state(sa, sb, but=("built_by",))


# ---- GPU (b): non-finite vertices --------------------------------------------------------------------------------------------------------------------------

NON_FINITE = [(65, None), (1025, 1), (4099, None)]


@gpu
@pytest.mark.parametrize("n,axis", NON_FINITE, ids=[f"{n}{'' if a is None else '-axis' + str(a)}" for n, a in NON_FINITE])
@pytest.mark.parametrize("method", METHODS)
def test_non_finite_vertices_build_update_and_sparse_update(native, method, n, axis):
    """About 2 % of the triangles carry NaN, +inf or -inf (1025: the whole y axis is NaN too).  The build, then a plain update and a sparse update that move
    non-finite values in and out, against the numpy statements: rvpt_build.h's "a NaN takes no part" throughout."""
    from rvpt_amd import scene
    base = ds.soup(n, 7000 + n)
    tris, pick0 = ds.with_non_finite(base, 1, whole_axis=axis)
    assert ds.no_zero_coordinate(tris)
    with np.errstate(all="ignore"):
        nodes, perm, tree = numpy_tree(method, tris)[:3]
        exp = ds.Expected(nodes, breadth_first=True)
    what = f"{method} {n} non-finite"
    with lab_context(native) as ctx:
        assert ctx.build_scene(tris, materials(), method=method) == tree
        s0 = ctx.scene_state()
        check_build_state(s0, tris, nodes, perm, exp, method, what + ": build", nan=True)
        # the plain update: another set of triangles is non-finite, the old ones are finite again
        moved, pick1 = ds.with_non_finite(base, 2, whole_axis=None if axis is None else (axis + 1) % 3)
        assert not np.array_equal(pick0, pick1)
        with np.errstate(all="ignore"):
            refit = scene.refit_bvh(nodes, moved[perm])
        ctx.update_triangles(moved)
        s1 = ctx.scene_state()
        dev1 = ds.shifted_layout(refit)
        assert ds.same_nodes(s1["nodes"], dev1, True), (what, "update: d_nodes", ds.first_difference(s1["nodes"], dev1))
        assert ds.same_bytes(s1["tris"][:, :12], moved[perm][:, :12]) and ds.same_bytes(s1["tris"][:, 12:], tris[perm][:, 12:]), what
        assert same_wide(s1["wide"], ds.regathered(exp.wide, s0["wide_map"], dev1)), what
        ds.check_wide_map(s1, what + ": update")
        # the sparse update: both sets and a few more take the rows of a third variant
        third, pick2 = ds.with_non_finite(base, 3)
        idx = np.unique(np.concatenate([pick0, pick1, pick2, np.arange(0, n, 11)]))
        patched = moved.copy()
        patched[idx, :12] = third[idx, :12]
        inv = np.argsort(perm)
        with np.errstate(all="ignore"):
            refit2 = scene.refit_bvh(refit, patched[perm], touched=inv[idx])
        ctx.update_triangles(patched[idx], indices=idx)
        s2 = ctx.scene_state()
        dev2 = ds.shifted_layout(refit2)
        assert ds.same_nodes(s2["nodes"], dev2, True), (what, "sparse update: d_nodes", ds.first_difference(s2["nodes"], dev2))
        assert ds.same_bytes(s2["tris"][:, :12], patched[perm][:, :12]) and ds.same_bytes(s2["tris"][:, 12:], tris[perm][:, 12:]), what
        assert same_wide(s2["wide"], ds.regathered(exp.wide, s0["wide_map"], dev2)), what
        assert s2["have_sparse_maps"] and not s2["sparse_dirty"].any() and ds.same_bytes(s2["inv_perm"], inv.astype(np.uint32)), what


@gpu
def test_sah_centroid_bounds_of_nothing_but_infinity(native):
    """tests/test_sah_host.py's infinite axis: every x is +inf.  The host's Box gives the root the centroid bounds [FLT_MAX, +inf] on x, the widest axis, and the
    median split keeps the caller's order; a device that reduced to lo = +inf would sort by y and hand the children the other halves."""
    from test_sah_host import infinite_axis
    tris = infinite_axis()
    assert ds.no_zero_coordinate(tris)
    with np.errstate(all="ignore"):
        nodes, perm, tree = numpy_tree("sah", tris)[:3]
        exp = ds.Expected(nodes, breadth_first=True)
    with lab_context(native) as ctx:
        assert ctx.build_scene(tris, materials(), method="sah") == "sah"
        check_build_state(ctx.scene_state(), tris, nodes, perm, exp, "sah", "sah, x all +inf", nan=True)


# ---- GPU (c): the plain update ---------------------------------------------------------------------------------------------------------------------------------

def host_tree(name):
    """(tris in leaf order, caller's nodes) of the trees the update forms start from"""
    from rvpt_amd import native as nat, scene
    if name in ("default", "loose"):
        tris, _ = scene.default_scene()
        nodes, idx = nat.build_bvh(tris)
        return tris[idx], (_loosen_boxes(nodes, 5) if name == "loose" else nodes)
    if name == "soup4099":
        tris = ds.soup(4099, 4099)
        nodes, idx = nat.build_bvh(tris)
        return tris[idx], nodes
    tris = ds.soup(143, 143)
    if name == "chain":
        tris = tris[:64].copy()
        return tris, _chain_bvh(tris)
    assert name == "two_leaves"
    return tris, scene.refit_bvh(_two_leaf_tree(tris), tris)


def extent(tris):
    return float(np.ptp(ds.vertices(tris).reshape(-1, 3), axis=0).max())


WIDE_FORM_COMPARED = {False: 0, True: 0}  # updates whose d_wide was / was not also compared with a fresh wide form of the refit tree


def check_update_state(before, after, exp, want_nodes, want_vertices, what):
    """after an update of any form: the refit's boxes, the upload's wide grouping with those boxes gathered, new vertices beside the stored material rows, and
    everything that follows from the topology alone as it was"""
    dev, _ = ds.device_layout(want_nodes)
    assert ds.same_nodes(after["nodes"], dev), (what, "d_nodes", ds.first_difference(after["nodes"], dev))
    want_wide = ds.regathered(before["wide"], before["wide_map"], dev)
    assert ds.same_bytes(after["wide"], want_wide), (what, "d_wide", ds.first_difference(after["wide"], want_wide))
    fresh, _ = ds.native.wide_form(dev, exp.head_shift)
    # A fresh regrouping of the refit tree opens the child with the largest box first and may group differently (tests/test_refit_host.py); the device keeps the
    # upload's grouping, which the comparison above and check_wide_map below pin.  Where the fresh form has the same heads throughout it is compared whole as
    # well; where not, that is counted and printed, never silent.  (A prefix cannot be compared instead: slots that are all inner carry consecutive wide
    # indices as heads whichever binary nodes stand behind them.)  On the MI355X 5 of the file's 46 updates keep every head.
    regrouped = not (fresh.shape == want_wide.shape and ds.same_bytes(fresh[:, 6:, :], want_wide[:, 6:, :]))
    WIDE_FORM_COMPARED[regrouped] += 1
    print(f"{what}: d_wide against the wide form of the refit tree: {'NOT compared, a fresh regrouping has other heads' if regrouped else 'equal heads, compared'} "
          f"(so far {WIDE_FORM_COMPARED[False]} compared, {WIDE_FORM_COMPARED[True]} not)")
    if not regrouped:
        assert ds.same_bytes(after["wide"], fresh), (what, "d_wide against the wide form of the refit tree")
    ds.check_wide_map(after, what)
    assert ds.same_bytes(after["tris"][:, :12], want_vertices[:, :12]), (what, "d_tris bytes 0-47")
    assert ds.same_bytes(after["tris"][:, 12:], before["tris"][:, 12:]), (what, "d_tris bytes 48-63")
    for k in ("wide_map", "refit_levels", "perm", "n_tris", "n_nodes", "n_wide", "bvh_height", "bvh_head_shift", "wide_stack_levels", "built_by", "have_perm"):
        assert ds.same_bytes(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k], (what, k)


@gpu
@pytest.mark.parametrize("name", ["default", "soup4099", "chain", "two_leaves", "loose"])
def test_plain_update_state_is_the_refit(native, name):
    from rvpt_amd import scene
    tris, nodes = host_tree(name)
    exp = ds.Expected(nodes)
    if name == "chain":
        assert exp.height == 64
    with lab_context(native) as ctx:
        ctx.upload_scene(nodes, tris, materials())
        s0 = ctx.scene_state()
        check_tree_state(s0, exp, name)
        assert ds.same_bytes(s0["tris"], tris) and s0["built_by"] is None and not s0["have_perm"] and s0["perm"].size == 0
        assert cost_close(s0["base_cost"], scene.tree_cost(nodes))
        for phase in (0.7, 1.9):
            moved = scene.wobble(tris, phase, 0.1 * extent(tris))
            assert ds.no_zero_coordinate(moved)
            moved[:, 12:] = 77.0  # the material row of the source is not read
            ctx.update_triangles(moved)
            check_update_state(s0, ctx.scene_state(), exp, scene.refit_bvh(nodes, moved), moved, f"{name} phase {phase}")


# ---- GPU (d): shrinking moves — the case images cannot see -----------------------------------------------------------------------------------------------------

def strictly_inside_somewhere(new, old, which):
    """of the numpy results: every box `which` lies inside its old box and strictly so on at least one bound"""
    a, b = new["bounds"][which], old["bounds"][which]
    inside = (a[:, 0::2] >= b[:, 0::2]).all(axis=1) & (a[:, 1::2] <= b[:, 1::2]).all(axis=1)
    strict = (a[:, 0::2] > b[:, 0::2]).any(axis=1) | (a[:, 1::2] < b[:, 1::2]).any(axis=1)
    return bool(inside.all() and strict.all())


def whole_leaves(nodes, every):
    """(leaf nodes, the positions of all their triangles) of every `every`-th leaf of a tree in the caller's layout"""
    rec = np.ascontiguousarray(nodes).view(ds.NODE).reshape(-1)
    leaves = np.flatnonzero(rec["count"] > 0)[::every]
    return leaves, np.concatenate([np.arange(rec["first"][l], rec["first"][l] + rec["count"][l]) for l in leaves])


def path_nodes(nodes, leaves):
    """the nodes between `leaves` and the root, both included, in the caller's layout"""
    rec = np.ascontiguousarray(nodes).view(ds.NODE).reshape(-1)
    parent = np.full(rec.shape[0], -1, dtype=np.int64)
    inner = np.flatnonzero(rec["count"] == 0)
    parent[rec["first"][inner]], parent[rec["first"][inner] + 1] = inner, inner
    on = np.zeros(rec.shape[0], dtype=bool)
    for l in leaves:
        while l >= 0 and not on[l]:
            on[l] = True
            l = parent[l]
    return on


@gpu
@pytest.mark.parametrize("form", ["plain", "sparse"])
@pytest.mark.parametrize("source", ["upload", "lbvh", "ploc", "sah"])
def test_shrinking_triangles_shrink_their_leaves_and_ancestors(native, source, form):
    """Every touched triangle scaled by 0.5 towards its own centroid: the image of a tree that kept the old, larger boxes would be the same.  Plain: all
    triangles; sparse: the triangles of every third leaf, whole leaves."""
    from rvpt_amd import native as nat, scene
    n = 1025
    if source == "upload":
        base = ds.soup(n, 88)
        nodes, order = nat.build_bvh(base)
        tris, perm = base, order  # the caller of upload_scene passes leaf order: positions are indices
        nodes = np.ascontiguousarray(nodes).view(ds.NODE).reshape(-1)
    else:
        tris, nodes, perm, _, _ = tree_of(source, "soup", n)
    leaf_order = tris[perm]
    exp = ds.Expected(nodes, breadth_first=source != "upload")
    every = 1 if form == "plain" else 3
    leaves, pos = whole_leaves(nodes, every)
    small = ds.shrunk(leaf_order, pos)
    assert ds.no_zero_coordinate(small)
    want = scene.refit_bvh(nodes, small, touched=None if form == "plain" else pos)
    assert strictly_inside_somewhere(want, nodes, leaves)
    if form == "plain":
        assert strictly_inside_somewhere(want, nodes, np.arange(len(nodes)))  # every ancestor too, the root included
    else:
        on = path_nodes(nodes, leaves)
        above = on & (nodes["count"] == 0)
        assert ds.same_bytes(want["bounds"][~on], nodes["bounds"][~on]) and not ds.same_bytes(want["bounds"][above], nodes["bounds"][above])
    with lab_context(native) as ctx:
        if source == "upload":
            ctx.upload_scene(nodes, leaf_order, materials())
            rows, idx = small, pos
        else:
            ctx.build_scene(tris, materials(), method=source)
            rows, idx = small[np.argsort(perm)], perm[pos]  # the caller's order
        s0 = ctx.scene_state()
        if form == "plain":
            ctx.update_triangles(rows)
        else:
            ctx.update_triangles(rows[idx], indices=idx)
        s1 = ctx.scene_state()
        check_update_state(s0, s1, exp, want, small, f"{source} {form} shrink")
        if form == "sparse":
            assert not s1["sparse_dirty"].any()


@gpu
def test_sparse_update_of_a_loosened_tree_leaves_the_other_boxes_as_they_were(native):
    from rvpt_amd import native as nat, scene
    base = ds.soup(1025, 89)
    tight, order = nat.build_bvh(base)
    tris = base[order]
    loose = _loosen_boxes(tight, 5)
    exp = ds.Expected(loose)
    leaves, pos = whole_leaves(loose, 5)
    small = ds.shrunk(tris, pos)
    want = scene.refit_bvh(loose, small, touched=pos)
    on = path_nodes(loose, leaves)
    assert not ds.same_bytes(loose["bounds"][~on], np.ascontiguousarray(tight).view(ds.NODE).reshape(-1)["bounds"][~on])  # loose boxes remain off the paths
    with lab_context(native) as ctx:
        ctx.upload_scene(loose, tris, materials())
        s0 = ctx.scene_state()
        check_tree_state(s0, exp, "loose upload")
        ctx.update_triangles(small[pos], indices=pos)
        s1 = ctx.scene_state()
        check_update_state(s0, s1, exp, want, small, "loose sparse shrink")
        # ... said once more in the device's own terms: off the touched paths the node bytes are those from before the call
        dev_on = np.zeros(exp.n_nodes, dtype=bool)
        for l in np.unique(exp.leaf_of[pos]):
            while l != ds.EMPTY and not dev_on[l]:
                dev_on[l] = True
                l = exp.parent[l]
        assert dev_on.sum() == on.sum()
        assert ds.same_bytes(s1["nodes"][~dev_on], s0["nodes"][~dev_on]) and not ds.same_bytes(s1["nodes"][dev_on], s0["nodes"][dev_on])
        assert not s1["sparse_dirty"].any()


# ---- GPU (e): the sparse update's bookkeeping -----------------------------------------------------------------------------------------------------------------

def index_lists(nodes, n):
    """one index; one whole leaf; every 7th; a shuffled third; all — as positions in leaf order"""
    rec = np.ascontiguousarray(nodes).view(ds.NODE).reshape(-1)
    leaf = np.flatnonzero(rec["count"] > 0)
    leaf = leaf[np.argmax(rec["count"][leaf])]
    rng = np.random.RandomState(7)
    return {"one": np.array([n // 2]), "leaf": np.arange(rec["first"][leaf], rec["first"][leaf] + rec["count"][leaf]), "every7th": np.arange(3, n, 7),
            "third": rng.permutation(n)[:n // 3], "all": np.arange(n)}


def displaced(tris, pos, phase):
    from rvpt_amd import scene
    out = tris.copy()
    out[pos, :12] = scene.wobble(tris, phase, 0.1 * extent(tris))[pos, :12]
    return out


def check_sparse_maps(state, exp, perm, what):
    assert state["have_sparse_maps"], what
    assert ds.same_bytes(state["sparse_parent"], exp.parent[:exp.n_map_nodes]), (what, "d_sparse_parent", ds.first_difference(state["sparse_parent"], exp.parent[:exp.n_map_nodes]))
    assert ds.same_bytes(state["sparse_leaf_of"], exp.leaf_of), (what, "d_sparse_leaf_of", ds.first_difference(state["sparse_leaf_of"], exp.leaf_of))
    assert state["sparse_dirty"].shape == (exp.n_map_nodes,) and not state["sparse_dirty"].any(), (what, "d_sparse_dirty", np.flatnonzero(state["sparse_dirty"]))
    if perm is None:
        assert not state["have_inv_perm"] and state["inv_perm"].size == 0, what
    else:
        assert state["have_inv_perm"] and ds.same_bytes(state["inv_perm"], np.argsort(perm).astype(np.uint32)), (what, "d_inv_perm")


@gpu
@pytest.mark.parametrize("source", ["upload", "lbvh", "ploc", "sah"])
def test_sparse_update_bookkeeping(native, source):
    """The five lists one after another on one context, then the refused lists of test_sparse_update.py (out of range, twice, too many): maps, inverse
    permutation, flags all zero after each, and nodes, triangles and wide bytes untouched by a refused call."""
    from rvpt_amd import native as nat, scene
    n = 4099
    if source == "upload":
        base = ds.soup(n, 90)
        nodes, order = nat.build_bvh(base)
        tris, perm = base[order], None
        nodes = np.ascontiguousarray(nodes).view(ds.NODE).reshape(-1)
    else:
        tris, nodes, perm, _, _ = tree_of(source, "soup", n)
    leaf_order = tris if perm is None else tris[perm]
    exp = ds.Expected(nodes, breadth_first=perm is not None)
    with lab_context(native) as ctx:
        if perm is None:
            ctx.upload_scene(nodes, tris, materials())
        else:
            ctx.build_scene(tris, materials(), method=source)
        s0 = ctx.scene_state()
        assert not s0["have_sparse_maps"] and not s0["have_inv_perm"]
        cur_nodes, cur = nodes, leaf_order
        for k, (name, pos) in enumerate(index_lists(nodes, n).items()):
            cur = displaced(cur, pos, 0.5 + k)
            assert ds.no_zero_coordinate(cur)
            cur_nodes = scene.refit_bvh(cur_nodes, cur, touched=pos)
            idx = pos if perm is None else perm[pos]
            ctx.update_triangles(cur[pos], indices=idx)
            s = ctx.scene_state()
            check_update_state(s0, s, exp, cur_nodes, cur, f"{source} list {name}")
            check_sparse_maps(s, exp, perm, f"{source} list {name}")
        assert cur_nodes.tobytes() == scene.refit_bvh(nodes, cur).tobytes()  # tight boxes: after "all" the sparse refit is the full one
        rows = np.ascontiguousarray(cur[:8])
        refused = [(np.array([5, n + 3, 9, n, 2]), rows[:5], "is outside"), (np.array([40, 9, 17, 40, 9, 3, 17, 100]), rows, "occurs more than once"),
                   (np.arange(n + 1), np.concatenate([cur, cur[:1]]), "the uploaded scene has")]
        for idx, r, said in refused:
            with pytest.raises(native.NativeError, match=said) as e:
                ctx.update_triangles(r, indices=idx)
            assert e.value.code == native.ERR_INVALID
            same_state(s, ctx.scene_state())  # nodes, triangles, wide bytes, maps, flags: nothing moved
            assert not ctx.scene_state(["sparse_dirty"])["sparse_dirty"].any()


@gpu
def test_a_rebuild_drops_the_maps_and_the_next_sparse_update_makes_the_new_trees(native):
    from rvpt_amd import scene
    a_tris, a_nodes, a_perm, _, a_exp = tree_of("lbvh", "soup", 1025)
    b_tris, b_nodes, b_perm, _, b_exp = tree_of("sah", "lattice", 2049)
    with lab_context(native) as ctx:
        ctx.build_scene(a_tris, materials(), method="lbvh")
        ctx.update_triangles(a_tris[:3], indices=np.arange(3))
        check_sparse_maps(ctx.scene_state(), a_exp, a_perm, "first tree")
        ctx.build_scene(b_tris, materials(), method="sah")
        s = ctx.scene_state()
        check_build_state(s, b_tris, b_nodes, b_perm, b_exp, "sah", "after the rebuild")  # (have_sparse_maps and have_inv_perm dropped, their pieces empty)
        idx = np.arange(5, 2049, 9)
        patched = displaced(b_tris, idx, 1.1)
        ctx.update_triangles(patched[idx], indices=idx)
        s1 = ctx.scene_state()
        check_sparse_maps(s1, b_exp, b_perm, "second tree")
        check_update_state(s, s1, b_exp, scene.refit_bvh(b_nodes, patched[b_perm], touched=np.argsort(b_perm)[idx]), patched[b_perm], "second tree")
        # a guarded update that rebuilds drops them too
        moved = scene.wobble(b_tris, 1.9, 0.3 * extent(b_tris))
        rep = ctx.update_triangles(moved, rebuild_above=1.0)
        assert rep.rebuilt
        s2 = ctx.scene_state()
        assert not s2["have_sparse_maps"] and not s2["have_inv_perm"] and s2["sparse_parent"].size == 0 and s2["inv_perm"].size == 0


@gpu
def test_twenty_thousand_scattered_indices_state(native):
    """test_sparse_update.py's 20 000 of 66 248 (heightfield_scene(182)): thousands of threads race to flag the upper levels.  The state only, no frame.  The
    terrain's vertices hold zeros on its border; the displaced ones and the wobbled boxes are compared with numpy all the same: a zero that ties with a zero of
    the other sign would show here as a sign bit and nowhere else."""
    from rvpt_amd import native as nat, scene
    tris, mats = scene.heightfield_scene(182)
    nodes, order = nat.build_bvh(tris)
    tris = tris[order]
    assert tris.shape[0] == 66248
    v = ds.vertices(tris)
    assert not (np.signbit(v) & (v == 0)).any()  # no -0: min / max cannot meet zeros of two signs
    exp = ds.Expected(nodes)
    idx = np.random.RandomState(31).permutation(tris.shape[0])[:20000]
    patched = displaced(tris, idx, 1.2)
    pv = ds.vertices(patched)
    assert not (np.signbit(pv) & (pv == 0)).any()
    with lab_context(native) as ctx:
        ctx.upload_scene(nodes, tris, mats)
        s0 = ctx.scene_state()
        ctx.update_triangles(patched[idx], indices=idx)
        s1 = ctx.scene_state()
        check_update_state(s0, s1, exp, scene.refit_bvh(nodes, patched, touched=idx), patched, "20 000 of 66 248")
        check_sparse_maps(s1, exp, None, "20 000 of 66 248")


# ---- GPU (f): the guarded update ---------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("method", METHODS)
def test_guarded_update_state(native, method):
    """Below the limit the state is the plain update's; above it, a fresh build_scene's of the moved triangles by the same method, d_perm and base cost included."""
    from rvpt_amd import scene
    tris, nodes, perm, tree, exp = tree_of(method, "soup", 1025)
    assert tree == method
    moved = scene.wobble(tris, 1.9, 0.3 * extent(tris))
    assert ds.no_zero_coordinate(moved)
    refit = scene.refit_bvh(nodes, moved[perm])
    ratio = scene.tree_cost(refit) / scene.tree_cost(nodes)
    assert 1.01 < ratio < 60.0, ratio  # between the two limits used below, clear of both
    with lab_context(native) as ctx, lab_context(native) as plain, lab_context(native) as fresh:
        ctx.build_scene(tris, materials(), method=method)
        plain.build_scene(tris, materials(), method=method)
        s0 = ctx.scene_state()
        rep = ctx.update_triangles(moved, rebuild_above=65.0)
        assert not rep.rebuilt
        plain.update_triangles(moved)
        s1 = ctx.scene_state()
        same_state(s1, plain.scene_state())
        check_update_state(s0, s1, exp, refit, moved[perm], f"{method} guarded, refitted")
        assert s1["base_cost"] == s0["base_cost"]
        rep = ctx.update_triangles(moved, rebuild_above=1.0)
        assert rep.rebuilt and rep.tree == method
        s2 = ctx.scene_state()
        assert fresh.build_scene(moved, materials(), method=method) == method
        same_state(s2, fresh.scene_state())
        new_nodes, new_perm = numpy_tree(method, moved)[:2]
        moved_rows = moved.copy()
        moved_rows[:, 12:] = tris[:, 12:]
        check_build_state(s2, moved_rows, new_nodes, new_perm, ds.Expected(new_nodes, breadth_first=True), method, f"{method} guarded, rebuilt")  # base_cost: the new tree's


# ---- GPU (g): the geometric ladder — the SAH build's rule "from depth 30 on, only median splits" -------------------------------------------------------------------

LADDER_ROWS = list(ds.LADDERS)
LADDER_IDS = ["-".join(map(str, r)) for r in LADDER_ROWS]
PLAIN_LADDER = LADDER_ROWS[0]  # (30, 300, 1): 330 triangles, 37 levels


def ladder_tree(method, row):
    """tree_of for ds.ladder(*row): (tris, nodes, perm, reported tree, ds.Expected, the builder's info) — built once, shared and left unchanged"""
    key = (method, "ladder", row)
    if key not in _TREES:
        tris = ds.ladder(*row)
        assert ds.no_zero_coordinate(tris)
        nodes, perm, tree, built = numpy_tree(method, tris)
        _TREES[key] = (tris, nodes, perm, tree, ds.Expected(nodes, breadth_first=True), built)
    return _TREES[key]


@gpu
@pytest.mark.parametrize("row", LADDER_ROWS, ids=LADDER_IDS)
def test_ladder_sah_build_state_is_the_numpy_statements(native, row):
    """sah_decide's `depth < kSahBalanceDepth` and sah_decide_level's skipped sah_large_bins, reached: thirty binned levels that peel one triangle each, then
    the cluster at depth 30 (29 for the third row, the other side of the comparison) — 5000 triangles are a large node whose bins nobody fills, nine are one
    median split, eight a leaf.  tests/test_sah_host.py holds the numpy tree to the table of ds.LADDERS and to rvpt_bvh_build's tree."""
    tris, nodes, perm, tree, exp, info = ladder_tree("sah", row)
    assert info == {k: v for k, v in ds.LADDERS[row].items() if k != "n"} and exp.height == info["height"]
    with lab_context(native) as ctx:
        assert ctx.build_scene(tris, materials(), method="sah") == "sah"
        state = ctx.scene_state()
        print(f"ladder {row}: n {tris.shape[0]} bvh_height {state['bvh_height']} wide_stack_levels {state['wide_stack_levels']} n_wide {state['n_wide']}")
        check_build_state(state, tris, nodes, perm, exp, "sah", f"sah ladder {row}")


@gpu
def test_hittable_ladder_sah_build_state_is_the_numpy_statements(native):
    """the ladder tests/test_ray_query.py sends rays down (ds.HITTABLE_LADDER): 17 between the rungs, not 32 — nearer to the edge of bin 15"""
    tris = ds.ladder(**ds.HITTABLE_LADDER)
    assert ds.no_zero_coordinate(tris)
    nodes, perm, _, info = numpy_tree("sah", tris)
    assert info == {k: v for k, v in ds.LADDERS[PLAIN_LADDER].items() if k != "n"}
    with lab_context(native) as ctx:
        assert ctx.build_scene(tris, materials(), method="sah") == "sah"
        check_build_state(ctx.scene_state(), tris, nodes, perm, ds.Expected(nodes, breadth_first=True), "sah", "sah hittable ladder")


@gpu
def test_ladder_sah_build_state_from_a_device_tensor(native):
    import torch
    tris, nodes, perm, tree, exp, _ = ladder_tree("sah", PLAIN_LADDER)
    with lab_context(native) as ctx:
        assert ctx.build_scene(torch.from_numpy(tris).to("cuda:0"), materials(), method="sah") == "sah"
        check_build_state(ctx.scene_state(), tris, nodes, perm, exp, "sah", f"sah ladder {PLAIN_LADDER} from a tensor")


@gpu
@pytest.mark.parametrize("row", LADDER_ROWS[:2], ids=LADDER_IDS[:2])
@pytest.mark.parametrize("method", ["lbvh", "ploc"])
def test_ladder_morton_build_state_is_the_numpy_statements(native, method, row):
    """The same input through the two Morton builders: an axis of 150 binades quantised to 10 bits leaves nearly every triangle in one cell"""
    tris, nodes, perm, tree, exp, _ = ladder_tree(method, row)
    assert tree == method  # (PLOC: no fallback)
    with lab_context(native) as ctx:
        assert ctx.build_scene(tris, materials(), method=method) == tree
        state = ctx.scene_state()
        print(f"ladder {row} {method}: bvh_height {state['bvh_height']} wide_stack_levels {state['wide_stack_levels']}")
        check_build_state(state, tris, nodes, perm, exp, method, f"{method} ladder {row}")


def ladder_rungs(tris, rungs=30):
    """the caller's indices of the `rungs` triangles furthest out"""
    return np.sort(np.argsort(tris[:, 0])[-rungs:])


@gpu
def test_plain_update_of_a_device_built_tree_of_37_levels(native):
    """Another ladder of the same size over the stored topology: the refit level table's 37 levels, deepest first"""
    from rvpt_amd import scene
    tris, nodes, perm, _, exp, _ = ladder_tree("sah", PLAIN_LADDER)
    moved = ds.ladder(30, 300, 11)
    assert moved.shape == tris.shape and ds.no_zero_coordinate(moved) and not ds.same_bytes(moved, tris)
    want = scene.refit_bvh(nodes, moved[perm])
    assert not ds.same_bytes(want["bounds"], nodes["bounds"])
    with lab_context(native) as ctx:
        ctx.build_scene(tris, materials(), method="sah")
        s0 = ctx.scene_state()
        assert s0["bvh_height"] == 37
        ctx.update_triangles(moved)
        check_update_state(s0, ctx.scene_state(), exp, want, moved[perm], "ladder plain update")


@gpu
def test_sparse_update_of_a_device_built_tree_of_37_levels(native):
    """The 30 rungs, their x scaled by 0.75 (exact), and 30 triangles of the cluster as they are: every leaf of the cluster lies 36 parents below the root, so
    the flag walk climbs 36 levels; the boxes of all 30 chain nodes change, the rest keep the bytes they had."""
    from rvpt_amd import scene
    tris, nodes, perm, _, exp, _ = ladder_tree("sah", PLAIN_LADDER)
    rungs = ladder_rungs(tris)
    others = np.setdiff1d(np.arange(tris.shape[0]), rungs)
    idx = np.concatenate([rungs, np.random.RandomState(5).permutation(others)[:30]])  # the caller's indices, in no order
    patched = tris.copy()
    patched[rungs, 0:12:4] *= np.float32(0.75)
    assert ds.no_zero_coordinate(patched) and np.array_equal(patched[rungs, 0].astype(np.float64), tris[rungs, 0].astype(np.float64) * 0.75)
    inv = np.argsort(perm)
    pos = inv[idx]
    want = scene.refit_bvh(nodes, patched[perm], touched=pos)
    # the walks, from the maps alone: the nodes on the touched paths and the longest climb
    on, longest = np.zeros(exp.n_nodes, dtype=bool), 0
    for leaf in np.unique(exp.leaf_of[pos]):
        steps, at = 0, exp.parent[leaf]
        on[leaf] = True
        while at != ds.EMPTY:
            on[at] = True
            steps, at = steps + 1, exp.parent[at]
        longest = max(longest, steps)
    assert longest == 36 == exp.height - 1
    with lab_context(native) as ctx:
        ctx.build_scene(tris, materials(), method="sah")
        s0 = ctx.scene_state()
        ctx.update_triangles(patched[idx], indices=idx)
        s1 = ctx.scene_state()
        check_update_state(s0, s1, exp, want, patched[perm], "ladder sparse update")
        check_sparse_maps(s1, exp, perm, "ladder sparse update")
        assert ds.same_bytes(s1["nodes"][~on], s0["nodes"][~on]), "boxes off the touched paths moved"
        chain = np.flatnonzero(on & (s0["nodes"]["count"] == 0))[:30]  # the 30 nodes above the cluster, root first
        assert (s1["nodes"]["bounds"][chain] != s0["nodes"]["bounds"][chain]).any(axis=1).all()


@gpu
def test_guarded_update_rebuilds_a_ladder_by_the_depth_rule(native):
    """The smallest limit there is, and a third ladder: the refitted tree costs more, the rebuild is reported, and the state is a fresh SAH build's of the new
    ladder — the depth rule reached through the rebuild path."""
    from rvpt_amd import scene
    tris, nodes, perm, _, exp, _ = ladder_tree("sah", PLAIN_LADDER)
    moved = ds.ladder(30, 300, 12)
    assert moved.shape == tris.shape and ds.no_zero_coordinate(moved)
    ratio = scene.tree_cost(scene.refit_bvh(nodes, moved[perm])) / scene.tree_cost(nodes)
    assert ratio > 1.01, ratio  # clear of the limit
    new_nodes, new_perm, _, info = numpy_tree("sah", moved)
    assert info["height"] > 31 and info["median_splits"] > 0 and info["binned_splits"] == 30
    with lab_context(native) as ctx:
        ctx.build_scene(tris, materials(), method="sah")
        rep = ctx.update_triangles(moved, rebuild_above=1.0)
        assert rep.rebuilt and rep.tree == "sah"
        moved_rows = moved.copy()
        moved_rows[:, 12:] = tris[:, 12:]  # an update keeps the stored material rows
        check_build_state(ctx.scene_state(), moved_rows, new_nodes, new_perm, ds.Expected(new_nodes, breadth_first=True), "sah", "ladder guarded, rebuilt")
