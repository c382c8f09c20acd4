"""Crossing queries without a GPU: the form's values and sentences in include/rvpt_hip.h and rvpt_amd/native.py; the statement of tests/_crossings.py
against a plain loop over all triangles, against _multi_hit's any-hit lists, and against the analytic counts of a cube and an icosphere; RVPT.inside and
RVPT.signed_distance composed from the statement's answers; the conditions on the GPU tests' inputs; the wrappers refuse what they can see to be wrong."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _crossings as cr
import _multi_hit as mh
import _ray_query as rq

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rvpt_hip.h"
PINNED_UNKNOWN = (7, 15, 26, 27, 32, 41, 48, 57, 77)


def test_the_header_compiles_as_c99_with_the_struct_the_dtype_mirrors(tmp_path):
    from rvpt_amd import native
    dt = native.RAY_CROSSINGS_DTYPE
    assert dt.itemsize == 48 and dt.names == ("org", "tmax", "dir", "flags", "front", "back", "t_near", "t_far")
    assert dt.names[:4] == native.RAY_HIT_DTYPE.names[:4] and all(dt.fields[n][:2] == native.RAY_HIT_DTYPE.fields[n][:2] for n in dt.names[:4])
    offsets = "".join(f"assert(offsetof(rvpt_ray_crossings, {name}) == {dt.fields[name][1]});" for name in dt.names)
    assert [dt.fields[n][1] for n in dt.names] == [0, 12, 16, 28, 32, 36, 40, 44]
    src = ('#include "rvpt_hip.h"\n#include <assert.h>\n#include <stddef.h>\nint main(void){assert(RVPT_HIP_FORMAT_RAY_CROSSINGS == 8);'
           f"assert(sizeof(rvpt_ray_crossings) == 48);assert(sizeof(rvpt_ray_crossings) == sizeof(rvpt_ray_hit));{offsets}"
           "assert(sizeof(((rvpt_ray_crossings *)0)->front) == 4 && sizeof(((rvpt_ray_crossings *)0)->t_far) == 4);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)


def test_the_bindings_values_and_the_formats_that_stay_unknown():
    from rvpt_amd import native
    assert native.ABI_VERSION == 8 and len(native.EXPORTS) == 30
    assert native.FORMAT_RAY_CROSSINGS == 8 and native.FORMAT_RAY_CROSSINGS not in PINNED_UNKNOWN
    assert re.search(r"#define RVPT_HIP_FORMAT_RAY_CROSSINGS 8\b", HEADER.read_text())
    ctx = native.Context.__new__(native.Context)  # (_frame_buffer decides on the format before it looks at anything else)
    ctx.width, ctx.height, ctx.device = 8, 8, 0
    buf = np.zeros((8, 8, 4), np.float32)
    with pytest.raises(native.NativeError, match="read_into: format 8 holds query records, not a frame: use count_crossings_into"):
        ctx._frame_buffer(buf, 8, "read_into")
    for fmt in PINNED_UNKNOWN + (4,):
        with pytest.raises(native.NativeError, match=f"unknown format {fmt}$"):
            ctx._frame_buffer(buf, fmt, "read_into")
    with pytest.raises(native.NativeError, match="use trace_rays_into / trace_paths_into"):
        ctx._frame_buffer(buf, 2, "read_into")


def test_the_headers_sentences():
    raw = HEADER.read_text()
    version_comment = raw[:raw.index("/* ---- POD layouts")]
    assert re.search(r"Still 8, no new symbol: rvpt_hip_read with\s+the\s+format\s+RVPT_HIP_FORMAT_RAY_CROSSINGS\s+\(8\)\s+—\s+until\s+then\s+the\s+\"unknown\s+format\"\s+error\s+—\s+is\s+a\s+CROSSING\s+QUERY",
                     version_comment)
    text = " ".join(raw.replace(" * ", " ").split())
    assert "Format 26 and every other value are the \"unknown format\" error." in text  # the pinned sentences stay where they are
    assert text.index("K-NEAREST RAY QUERIES — the first k hits") < text.index("RAY CROSSINGS — how many surfaces") < text.index("PATH QUERIES — radiance along")
    for sentence in ("flags is reserved and ignored, RVPT_HIP_RAY_ANY_HIT included",
                     "is answered as a ray with no crossing.",
                     "THE SET A is every triangle test accepted by the walk of an any-hit k-nearest ray query with no limit on k.",
                     "`bound` stays tmax from start to end: every box test and every triangle test uses the interval (0, tmax)",
                     "a triangle is accepted iff 0 < t < tmax, 0 < u, 0 < v and u + v < 1.",
                     "A DOES NOT DEPEND ON THE VISITING ORDER, because the interval never changes: the answer is the same under RVPT_HIP_TRAVERSAL_BVH, "
                     "RVPT_HIP_TRAVERSAL_BVH_ORDERED and RVPT_HIP_BVH_PER_LANE.",
                     "Stacked duplicates count once each.",
                     "a caller's tree that lists a triangle under two leaves counts it twice.",
                     "s = (dir.x*n.x + dir.y*n.y) + dir.z*n.z in binary32, every operation rounded on its own, no FMA.",
                     "The hit is FRONT iff s < 0; every other hit is BACK (s > 0, s == 0, s NaN), hence front + back == |A|.",
                     "back - front is 1 from inside and 0 from outside along any ray that meets no edge exactly.",
                     "If A is empty: front = back = 0, t_near = the bits of tmax as given (a NaN's payload included), t_far = +0.0.",
                     "On brute-force contexts t_near equals format 2's t.",
                     "a box test may turn away a ray that its triangle's test would accept.",
                     "A finite tmax is the caller's bound.",
                     "for host records only the out quad travels back",
                     "DESIGN.md 5.27 has the kernels and what was measured (profiles/ray_crossings.txt)."):
        assert sentence in text, sentence


@pytest.fixture(scope="module")
def default_records(oracle, default_scene):
    """about 330 records of the default scene: base rays, their tmax variants, non-finite records"""
    tris, _, nodes = default_scene
    base = rq.base_rays(tris, 7, counts=(40, 40, 15, 10, 10, 5))
    st = rq.Statement(oracle, nodes, tris)
    return cr.records_of(np.concatenate([rq.with_tmax_variants(base, st.answer(base)), rq.non_finite_records(base, 9, 12)]))


def test_brute_force_order_is_a_plain_loop_over_all_triangles(oracle, default_scene, default_records):
    """Traversal 1: front, back, t_near, t_far from oracle_tri_test over every triangle with (0, tmax), the facing written out once more here"""
    from rvpt_amd import scene
    tris, _, nodes = default_scene
    st = cr.Statement(oracle, nodes, tris)
    n = scene.triangle_unit_normals(tris)
    got = st.answer_crossings(default_records, 1)
    counted = 0
    for k, r in enumerate(default_records):
        valid = np.isfinite(r["org"]).all() and np.isfinite(r["dir"]).all() and r["tmax"] > 0
        front = back = 0
        ts = []
        if valid:
            st._o[:], st._d[:] = r["org"], r["dir"]
            d = r["dir"]
            with np.errstate(all="ignore"):
                for i in range(st.n_tris):
                    if st._tri(i, float(r["tmax"])):
                        ts.append(st._tuv[0].copy())
                        s = np.float32(np.float32(d[0] * n[i, 0]) + np.float32(d[1] * n[i, 1])) + np.float32(d[2] * n[i, 2])
                        if s < 0:
                            front += 1
                        else:
                            back += 1
        g = got[k]
        assert (g["front"], g["back"]) == (front, back), k
        if ts:
            assert g["t_near"] == min(ts) and g["t_far"] == max(ts) and 0 < g["t_near"] <= g["t_far"] < r["tmax"]
            counted += 1
        else:
            assert g["t_near"].tobytes() == r["tmax"].tobytes() and g["t_far"].tobytes() == np.float32(0).tobytes()
    assert counted > 100 and (got["front"] > 0).sum() > 50 and (got["back"] > 0).sum() > 50 and ((got["front"] + got["back"]) >= 3).sum() > 5
    for name in ("org", "tmax", "dir", "flags"):
        assert got[name].tobytes() == default_records[name].tobytes()


def test_the_statement_against_the_any_hit_lists(oracle, default_scene, default_records):
    """Both orders: where the count is at most 8, the any-hit list of k = 8 has that length, and its min and max t are t_near and t_far.  The BVH order's
    counts equal the brute-force order's on these rays"""
    tris, _, nodes = default_scene
    st = cr.Statement(oracle, nodes, tris)
    answers = {}
    for traversal in (0, 1):
        got = answers[traversal] = st.answer_crossings(default_records, traversal)
        short = 0
        for k, r in enumerate(default_records):
            H = st.trace_k(r["org"], r["dir"], 8, r["tmax"], True, traversal)
            total = int(got["front"][k]) + int(got["back"][k])
            if total <= 8:
                assert len(H) == total
                short += 1
                if H:
                    assert min(h[1] for h in H) == got["t_near"][k] and max(h[1] for h in H) == got["t_far"][k]
            else:
                assert len(H) == 8
        assert short > 300
    assert rq.same_bytes(answers[0], answers[1])


SHAPES = {"cube": (cr.cube_scene, 2.0), "icosphere": (cr.icosphere_scene, 2.0)}


def probe_points(name, seed=3, n=40):
    """(points float32[2 n, 3], truth bool[2 n]): n inside and n outside, every one at least 0.05 of the extent (2) from the surface"""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(2 * n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if name == "cube":  # the cube [-1, 1]^3: inside max |x| <= 0.85, outside a point of a shell 1.15 .. 2 scaled by its largest coordinate
        inside = rng.uniform(-0.85, 0.85, (n, 3))
        outside = d[n:] / np.abs(d[n:]).max(axis=1, keepdims=True) * rng.uniform(1.15, 2.0, (n, 1))
    else:  # the icosphere's faces lie between radius 0.93 and 1
        inside = d[:n] * rng.uniform(0.0, 0.8, (n, 1))
        outside = d[n:] * rng.uniform(1.15, 2.0, (n, 1))
    return np.concatenate([inside, outside]).astype(np.float32), np.arange(2 * n) < n


@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_closed_shapes_give_the_analytic_counts(oracle, name):
    """From outside through the shape: 1 front + 1 back; from inside: 1 back; beside it: nothing.  Both orders"""
    from rvpt_amd import native, scene
    tris = SHAPES[name][0]()
    assert tris.shape[0] == {"cube": 12, "icosphere": 80}[name]
    n = scene.triangle_unit_normals(tris)
    centroid = tris.reshape(-1, 16)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).mean(axis=1)
    assert ((n * centroid).sum(axis=1) > 0).all()  # outward
    nodes, idx = native.build_bvh(tris)
    sorted_tris = np.ascontiguousarray(tris[idx])
    points, truth = probe_points(name)
    rng = np.random.RandomState(5)
    d = rng.normal(size=(points.shape[0], 3)) + 0.01
    outside = points[~truth]
    through = cr.make_records(outside, -outside.astype(np.float64) + rng.uniform(-0.2, 0.2, outside.shape))  # aimed near the centre
    from_inside = cr.make_records(points[truth], d[truth])
    away = cr.make_records(outside, outside)
    for st, traversal in ((cr.Statement(oracle, nodes, sorted_tris), 0), (cr.Statement(oracle, None, tris), 1)):
        got = st.answer_crossings(through, traversal)
        assert (got["front"] == 1).all() and (got["back"] == 1).all() and (got["t_near"] < got["t_far"]).all()
        got = st.answer_crossings(from_inside, traversal)
        assert (got["front"] == 0).all() and (got["back"] == 1).all() and (got["t_near"] == got["t_far"]).all()
        got = st.answer_crossings(away, traversal)
        assert (got["front"] == 0).all() and (got["back"] == 0).all() and np.isinf(got["t_near"]).all() and (got["t_far"].view(np.uint32) == 0).all()


def test_the_flipped_layers_and_a_tmax_exactly_on_a_layer(oracle):
    """256 through rays and their reverses: 12 crossings each, both facings on every ray, front and back trading places on the way back; the four duplicate
    layers are counted; tmax between two layers cuts the rest off, and tmax exactly at a layer's t does not count that layer (the test is strict)"""
    tris, zs = cr.flipped_layered_scene()
    st = cr.Statement(oracle, None, tris)
    rays = cr.records_of(mh.through_rays(256, 23))
    fwd = st.answer_crossings(rays, 1)
    assert (fwd["front"] + fwd["back"] == mh.LAYERS).all() and (fwd["front"] > 0).all() and (fwd["back"] > 0).all()
    assert len(set(zs)) == mh.LAYERS - len(mh.DUPLICATED)
    back = st.answer_crossings(cr.reversed_rays(rays, 8.0), 1)
    assert (back["front"] == fwd["back"]).all() and (back["back"] == fwd["front"]).all()
    some = rays[:32]
    full = st.answer_crossings(some, 1)
    for j, r in enumerate(some):
        H = sorted(st.trace_k(r["org"], r["dir"], cr.NO_LIMIT, np.inf, True, 1), key=lambda h: h[1])
        ts = sorted(set(h[1] for h in H))
        assert len(H) == 12 and len(ts) == 8
        on = r.copy()
        on["tmax"] = ts[3]  # exactly on the fourth distinct layer
        got = st.crossings(on["org"], on["dir"], on["tmax"], 1)
        below = sum(1 for h in H if h[1] < ts[3])
        assert got[0] + got[1] == below and got[3] == ts[2] and got[3] < on["tmax"]
        between = np.float32((np.float64(ts[3]) + np.float64(ts[4])) / 2)
        got = st.crossings(r["org"], r["dir"], between, 1)
        assert got[0] + got[1] == sum(1 for h in H if h[1] <= ts[3]) and got[3] == ts[3] and got[2] == full["t_near"][j]


def test_invalid_rays_and_a_nan_payload(oracle, default_scene):
    tris, _, nodes = default_scene
    st = cr.Statement(oracle, nodes, tris)
    base = rq.base_rays(tris, 7, counts=(20, 20, 0, 0, 0, 0))
    records = cr.records_of(np.concatenate([rq.non_finite_records(base, 9, 12), base[:8]]))
    records["tmax"][12:20] = [0.0, -0.0, -1.0, -np.inf, np.nan, np.nan, np.nan, np.nan]
    records["tmax"].view(np.uint32)[17:20] = [0x7FC12345, 0xFFC00001, 0x7F800001]  # quiet, negative and signalling NaNs: the payload comes back
    for traversal in (0, 1):
        got = st.answer_crossings(records, traversal)
        assert not got["front"].any() and not got["back"].any() and not got["t_far"].view(np.uint32).any()
        assert got["t_near"].tobytes() == records["tmax"].tobytes()
        assert got["t_near"].view(np.uint32)[17:20].tolist() == [0x7FC12345, 0xFFC00001, 0x7F800001]


def test_the_wrappers_refuse_what_they_can_see():
    import torch
    from rvpt_amd import native, renderer
    ctx = native.Context.__new__(native.Context)
    ctx.device = 0
    with pytest.raises(native.NativeError, match="count_crossings: 3 origins, 2 directions"):
        ctx.count_crossings(np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(native.NativeError, match="count_crossings: 3 rays, tmax of shape \\(2,\\)"):
        ctx.count_crossings(np.zeros((3, 3)), np.ones((3, 3)), tmax=np.ones(2))
    with pytest.raises(native.NativeError, match="count_crossings_into: a contiguous writeable RAY_CROSSINGS_DTYPE array is needed, got"):
        ctx.count_crossings_into(np.zeros(4, dtype=native.RAY_HIT_DTYPE))
    with pytest.raises(native.NativeError, match="count_crossings_into: a contiguous writeable RAY_CROSSINGS_DTYPE array is needed"):
        ctx.count_crossings_into(np.zeros(8, dtype=native.RAY_CROSSINGS_DTYPE)[::2])
    with pytest.raises(native.NativeError, match="count_crossings_into: a contiguous float32 tensor \\[n, 12\\] is needed"):
        ctx.count_crossings_into(torch.zeros(4, 11))
    with pytest.raises(native.NativeError, match="count_crossings_into: a contiguous float32 tensor \\[n, 12\\] is needed"):
        ctx.count_crossings_into(torch.zeros(4, 12, dtype=torch.float64))
    with pytest.raises(native.NativeError, match="a numpy array or a torch tensor is needed, got list"):
        ctx.count_crossings_into([1, 2])
    r = renderer.RVPT(8, 8)
    with pytest.raises(RuntimeError, match="count_crossings before initialize"):
        r.count_crossings(np.zeros((1, 3)), np.ones((1, 3)))
    with pytest.raises(ValueError, match="rule must be 'winding' or 'parity'"):
        r.inside(np.zeros((1, 3)), rule="odd")
    with pytest.raises(RuntimeError, match="count_crossings before initialize"):
        r.inside(np.zeros((1, 3)))


def test_the_three_directions():
    from rvpt_amd import renderer
    d = np.asarray(renderer.INSIDE_DIRECTIONS)
    assert d.shape == (3, 3) and (np.abs(d) > 0.2).all()  # none axis-aligned, none in a coordinate plane
    assert np.linalg.matrix_rank(d) == 3
    for row in d:
        assert ", ".join(f"{x}" for x in row) in renderer.RVPT.inside.__doc__  # written once in the module and in the docstring
    org, dirv = renderer.crossing_rays([[1, 2, 3], [4, 5, 6]])
    assert org.dtype == dirv.dtype == np.float32 and org.tolist() == [[1, 2, 3]] * 3 + [[4, 5, 6]] * 3 and np.array_equal(dirv, np.tile(d.astype(np.float32), (2, 1)))
    # two of three decide
    f = np.array([0, 0, 1, 0, 1, 1], np.uint32)
    b = np.array([1, 1, 1, 1, 1, 1], np.uint32)
    assert renderer.inside_from_crossings(f, b, "winding").tolist() == [True, False]
    assert renderer.inside_from_crossings(f, b, "parity").tolist() == [True, False]
    assert renderer.inside_from_crossings([2, 2, 2], [3, 3, 1], "winding").tolist() == [True]  # (unsigned counts do not wrap)
    assert renderer.inside_from_crossings([2, 2, 2], [3, 3, 1], "parity").tolist() == [True]


@pytest.mark.parametrize("name", ["cube", "icosphere"])
def test_inside_and_signed_distance_from_the_statements_answers(oracle, name):
    """RVPT.inside and RVPT.signed_distance composed from the statement's answers for the points the GPU tests use — and the conditions those tests rest on: all
    three directions give every point the same winding, and every point lies at least 0.05 of the extent from the surface"""
    from rvpt_amd import native, renderer, scene
    tris = SHAPES[name][0]()
    extent = SHAPES[name][1]
    points, truth = probe_points(name)
    st = cr.Statement(oracle, None, tris)
    org, dirv = renderer.crossing_rays(points)
    got = st.answer_crossings(cr.make_records(org, dirv), 1)
    winding = got["back"].astype(np.int64) - got["front"].astype(np.int64)
    assert (winding.reshape(-1, 3) == truth[:, None].astype(np.int64)).all()  # the same winding along all three directions, 1 inside and 0 outside
    for rule in ("winding", "parity"):
        assert np.array_equal(renderer.inside_from_crossings(got["front"], got["back"], rule), truth), rule
    near = scene.closest_points(tris, points)
    assert (near["prim"] != native.NO_PRIM).all() and (np.sqrt(near["d2"]) >= 0.05 * extent).all()
    sd = renderer.signed_distance_from(near["d2"], near["prim"], truth)
    assert sd.dtype == np.float32 and (sd[truth] < 0).all() and (sd[~truth] > 0).all() and np.array_equal(np.abs(sd), np.sqrt(near["d2"]))
    if name == "cube":  # the cube's distance is known in closed form
        p = np.abs(points.astype(np.float64))
        outside = np.linalg.norm(np.maximum(p - 1.0, 0.0), axis=1)
        want = np.where(truth, p.max(axis=1) - 1.0, outside)
        assert np.allclose(sd, want, rtol=1e-5, atol=1e-6)
    missed = renderer.signed_distance_from(np.float32([np.inf, 4.0]), np.uint32([native.NO_PRIM, 3]), [False, True])
    assert missed.tolist() == [np.inf, -2.0]
