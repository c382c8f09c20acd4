"""K-nearest point queries without a GPU: the form's values and sentences in include/rvpt_hip.h and rvpt_amd/native.py; the statement
rvpt_amd/scene.py: closest_points_k against closest_points (column 0, every k) and against a stable sort of all accepted candidates; NaN candidates; the
pruning rule in numpy over built and loose trees; the inputs shown to hold ties at every k; the wrappers refuse what they can see to be wrong before any call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _nearest as nq
import _nearest_k as nk

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "rvpt_hip.h"
KS = list(range(1, 9))


def test_the_header_compiles_as_c99_with_the_pinned_values(tmp_path):
    src = ('#include "rvpt_hip.h"\n#include <assert.h>\nint main(void){assert(RVPT_HIP_FORMAT_NEAREST_POINTS_K(1) == 49);assert(RVPT_HIP_FORMAT_NEAREST_POINTS_K(8) == 56);'
           "assert(RVPT_HIP_POINT_MAX_NEAREST == 8);assert(RVPT_HIP_FORMAT_NEAREST_POINTS_K(RVPT_HIP_POINT_MAX_NEAREST) == 56);assert(sizeof(rvpt_point_hit) == 48);"
           "assert(RVPT_HIP_FORMAT_NEAREST_POINTS == 4);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    subprocess.run([str(tmp_path / "t")], check=True)


def test_the_bindings_values_are_the_headers():
    from rvpt_amd import native, scene
    assert native.ABI_VERSION == 8 and len(native.EXPORTS) == 30
    assert native.POINT_MAX_NEAREST == 8 == scene.POINT_MAX_NEAREST
    assert [native.FORMAT_NEAREST_POINTS_K(k) for k in KS] == list(range(49, 57))
    assert native.FORMAT_NEAREST_POINTS_K(np.int64(3)) == 51
    text = HEADER.read_text()
    assert re.search(r"#define RVPT_HIP_POINT_MAX_NEAREST 8u\b", text) and re.search(r"#define RVPT_HIP_FORMAT_NEAREST_POINTS_K\(k\) \(48 \+ \(k\)\)", text)
    assert re.search(r"#define RVPT_HIP_ABI_VERSION 8\b", text)
    kernel_side = (ROOT / "rvpt_amd" / "csrc" / "rvpt_nearest.h").read_text()
    assert int(re.search(r"constexpr uint32_t kNearestMaxK = (\d+);", kernel_side).group(1)) == 8
    assert "static_assert(RVPT_HIP_POINT_MAX_NEAREST == rv::kNearestMaxK" in (ROOT / "rvpt_amd" / "csrc" / "rvpt_abi.hip").read_text()


def test_the_headers_sentences():
    raw = HEADER.read_text()
    version_comment = raw[:raw.index("/* ---- POD layouts")]
    assert re.search(r"Still 8, no new symbol: rvpt_hip_read with a format RVPT_HIP_FORMAT_NEAREST_POINTS_K\(k\) \(49 \.\. 56\)\s+—\s+until then the \"unknown format\" error\s+—\s+is a K-NEAREST POINT QUERY",
                     " ".join(version_comment.split()))
    text = " ".join(raw.replace(" * ", " ").split())
    assert "Format 26 and every other value are the \"unknown format\" error." in text  # the pinned sentences stay where they are
    assert text.index("NEAREST POINTS — the nearest point of the mesh") < text.index("K-NEAREST POINTS — the k nearest triangles") < text.index("TRIANGLES — the whole mesh as it now stands")
    for sentence in ("Record 0 of a group carries the point and the bound (point, max_d2); the in fields of records 1 .. k-1 are ignored.",
                     "No in field of any record is ever written.",
                     "The k belongs to the call, not to the record: a launch is uniform in k.",
                     "Formats 48 and 57 are the \"unknown format\" error.",
                     "a candidate whose d2 is NaN is never one.",
                     "The answer is the first k, in ascending lexicographic order of (d2, prim), of all candidates that are smaller than (max_d2, 0xFFFFFFFF).",
                     "when more than k candidates tie at the k-th distance the smaller numbers are the ones returned.",
                     "The answer is therefore the same after every builder.",
                     "the group holds EVERY triangle within the bound if its last slot is a miss, otherwise the k nearest of them.",
                     "From the first slot no candidate fills, every slot is a miss: closest = 0, 0, 0, d2 = the bits of record 0's max_d2 as given, prim = 0xFFFFFFFF, u = v = 0, region = 0.",
                     "gets k such slots, decided before any walk.",
                     "The empty scene answers every group so.",
                     "RVPT_HIP_FORMAT_NEAREST_POINTS_K(1) is format 4, the same kernels, the same bytes and the same messages.",
                     "A caller's tree that lists a triangle under two leaves may report it twice.",
                     "else RVPT_HIP_ERR_INVALID (the message gives k and the byte count)",
                     "untouched; host records go through the staging buffer and only the out fields travel back;"):
        assert sentence in text, sentence


@pytest.fixture(scope="module")
def default_candidates():
    """the default scene's 143 triangles, base_points(tris, 7) (916 points, unbounded) and every candidate's d2"""
    from rvpt_amd import scene
    tris = scene.default_scene()[0]
    base = nq.base_points(tris, 7)
    assert tris.shape[0] == 143 and base.shape[0] == 916
    d2 = scene.closest_point_triangles(base["point"], tris)[1]
    return tris, base, d2


def test_the_inputs_bite_at_every_k(default_candidates):
    """for every k = 1 .. 8 at least 100 of the 916 records have the k-th and the (k + 1)-th candidate at an equal d2: the cut at k goes through a tie, and
    only the order on prim decides who is returned"""
    _, _, d2 = default_candidates
    ordered = np.sort(d2, axis=1)
    counts = [int((ordered[:, k - 1] == ordered[:, k]).sum()) for k in KS]
    print("records with candidates k and k + 1 at an equal d2, k = 1 .. 8:", counts)
    assert all(c >= 100 for c in counts), counts


@pytest.mark.parametrize("k", KS)
def test_column_0_is_the_point_querys_statement_and_the_rows_a_stable_sort(default_candidates, k):
    from rvpt_amd import scene
    tris, base, d2 = default_candidates
    with np.errstate(all="ignore"):
        points = np.concatenate([nk.with_bound_variants_at(base[:60], tris, k), base[60:], nq.non_finite_records(base, 3, 12)])
        got = scene.closest_points_k(tris, points["point"], k, points["max_d2"])
        one = scene.closest_points(tris, points["point"], points["max_d2"])
    assert got.shape == (points.shape[0], k) and got.dtype == scene.POINT_HIT_DTYPE
    assert np.ascontiguousarray(got[:, 0]).tobytes() == one.tobytes()
    assert not got["point"][:, 1:].any() and not got["max_d2"][:, 1:].view(np.uint32).any()  # the in fields are column 0's
    # every row against a sort written out per point: all accepted candidates, ascending (d2, index), cut at k
    q, d2_all, u, v, region = scene.closest_point_triangles(points["point"], tris)
    short = 0
    for r in range(points.shape[0]):
        p, bound = points["point"][r], points["max_d2"][r]
        valid = bool(np.isfinite(p).all() and bound >= 0)
        with np.errstate(all="ignore"):
            idx = np.flatnonzero(d2_all[r] <= bound) if valid else np.zeros(0, np.int64)  # (false for a NaN d2)
        accepted = sorted(zip(d2_all[r, idx].tolist(), idx.tolist()))  # (tuples: by d2, then by index)
        row = got[r]
        for j in range(k):
            if j < len(accepted):
                i = accepted[j][1]
                assert row["prim"][j] == i and row["d2"][j].tobytes() == d2_all[r, i].tobytes() and row["closest"][j].tobytes() == q[r, i].tobytes()
                assert (row["u"][j], row["v"][j], row["region"][j]) == (u[r, i], v[r, i], region[r, i])
            else:
                assert row["prim"][j] == nq.NO_PRIM and row["d2"][j].tobytes() == bound.tobytes() and not row["closest"][j].any()
                assert row["u"][j] == 0 and row["v"][j] == 0 and row["region"][j] == 0
        short += 0 < len(accepted) < k
    if k > 1:
        assert short > 20  # radius queries that hold every triangle within their bound and end in misses


def test_a_nan_candidate_never_appears():
    """a triangle with a NaN vertex has a NaN d2: it is in no answer, at no k, though fewer than k others are in reach"""
    from rvpt_amd import scene
    tris = scene.default_scene()[0][:6].copy()
    tris[2, 4] = np.nan  # vert1.x of triangle 2
    pts = nq.base_points(scene.default_scene()[0][:6], 5, counts=(40, 6, 6, 6, 2))["point"]
    with np.errstate(all="ignore"):
        assert np.isnan(scene.closest_point_triangles(pts, tris)[1][:, 2]).all()
        got = scene.closest_points_k(tris, pts, 8)
    assert (got["prim"][:, :5] != nq.NO_PRIM).all() and (got["prim"][:, 5:] == nq.NO_PRIM).all() and not (got["prim"] == 2).any()
    assert np.isinf(got["d2"][:, 5:]).all() and not np.isnan(got["d2"]).any()


def test_k_outside_1_to_8_is_refused_by_the_statement():
    from rvpt_amd import scene
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            scene.closest_points_k(scene.default_scene()[0], np.zeros((1, 3)), k)


def _trees(tris, which):
    from rvpt_amd import native, scene
    nodes, perm = {"sah": scene.build_sah, "lbvh": scene.build_lbvh}[which if which != "grown" else "sah"](tris)[:2]
    if which == "grown":
        nodes = nq.grown_boxes(nodes, 4)
    return np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1), tris[perm]


@pytest.mark.parametrize("which", ["sah", "lbvh", "grown"])
def test_no_pruned_node_holds_a_member_of_the_answer(which):
    """The walk's rule in numpy: with bound_k the d2 of the k-th entry (max_d2 while the answer holds fewer), a node with box_d2 > bound_k — the final bound,
    the smallest the walk ever compares against — holds no member of the answer, over a built tree and over grown boxes; and nodes ARE pruned."""
    from rvpt_amd import scene
    tris = scene.default_scene()[0]
    nodes, stored = _trees(tris, which)
    base = nq.base_points(stored, 5, counts=(60, 20, 20, 20, 5))
    under = nq.triangles_under(nodes)
    for k in (1, 2, 5, 8):
        with np.errstate(all="ignore"):
            points = nk.with_bound_variants_at(base, stored, k)
            got = scene.closest_points_k(stored, points["point"], k, points["max_d2"])
        full = got["prim"][:, k - 1] != nq.NO_PRIM
        bound_k = np.where(full, got["d2"][:, k - 1], points["max_d2"])
        valid = np.isfinite(points["point"]).all(axis=1) & (points["max_d2"] >= 0)
        member = np.zeros((points.shape[0], tris.shape[0] + 1), bool)
        rows = np.repeat(np.arange(points.shape[0]), k)
        member[rows, np.minimum(got["prim"].reshape(-1), tris.shape[0])] = True  # (a miss goes to the spare column)
        pruned = 0
        for i, idx in under.items():
            with np.errstate(all="ignore"):
                skipped = valid & (scene.point_box_d2(points["point"], nodes["bounds"][i][0::2], nodes["bounds"][i][1::2]) > bound_k)
            assert not member[skipped][:, idx].any(), (which, k, i)
            pruned += int(skipped.sum())
        assert pruned > points.shape[0], (which, k)


def _context():
    from rvpt_amd import native
    ctx = object.__new__(native.Context)
    ctx._L, ctx._h = None, None
    ctx.device = 0
    return ctx


def test_the_wrappers_refuse_before_any_call():
    import torch
    from rvpt_amd import RVPT, native
    ctx = _context()
    good = np.zeros((4, 2), dtype=native.POINT_HIT_DTYPE)
    with pytest.raises(AttributeError):  # (the helper's premise: well-formed records do reach the call)
        ctx.closest_points_into(good, k=2)
    with pytest.raises(AttributeError):
        ctx.closest_points_into(good.reshape(-1), k=2)
    with pytest.raises(AttributeError):
        ctx.closest_points_into(torch.zeros((8, 12), dtype=torch.float32), k=2)
    with pytest.raises(AttributeError):
        ctx.closest_points(np.zeros((3, 3)), k=8)
    for bad in (0, 9, 2.5, "3", True, -1):
        for call in (lambda: ctx.closest_points(np.zeros((3, 3)), k=bad), lambda: ctx.closest_points_into(good, k=bad),
                     lambda: native.FORMAT_NEAREST_POINTS_K(bad), lambda: RVPT(8, 8).closest_points(np.zeros((3, 3)), k=bad)):
            with pytest.raises(native.NativeError, match=r"k must be an int in 1 \.\. 8") as e:
                call()
            assert e.value.code == native.ERR_INVALID
    for records in (np.zeros(7, dtype=native.POINT_HIT_DTYPE), torch.zeros((7, 12), dtype=torch.float32)):
        with pytest.raises(native.NativeError, match="7 records are not a multiple of k=2") as e:
            ctx.closest_points_into(records, k=2)
        assert e.value.code == native.ERR_INVALID
    for shape in ((3, 2), (2, 3, 3)):
        with pytest.raises(native.NativeError, match=r"k=3 needs POINT_HIT_DTYPE\[n, 3\]"):
            ctx.closest_points_into(np.zeros(shape, dtype=native.POINT_HIT_DTYPE), k=3)
    for bad in (np.zeros((4, 12), dtype=np.float32), torch.zeros((4, 11), dtype=torch.float32), "records"):  # the other refusals are closest_points_into's own
        with pytest.raises(native.NativeError) as e:
            ctx.closest_points_into(bad, k=2)
        assert e.value.code == native.ERR_INVALID and "closest_points_into" in str(e.value)
    with pytest.raises(RuntimeError, match="closest_points before initialize"):
        RVPT(8, 8).closest_points([0, 0, 0], k=2)


def test_rvpt_numbers_every_filled_slot_in_the_order_added():
    """RVPT.closest_points(k=) sends prim of every filled slot through primitive_indices after a host build and leaves the empty slots alone — against a
    recording stand-in for the context; without k the call goes out as before"""
    from rvpt_amd import RVPT, native

    class Recorder:
        def closest_points(self, points, max_dist, k=None):
            self.k = k
            n = np.asarray(points).reshape(-1, 3).shape[0]
            rec = np.zeros((n, k) if k else n, dtype=native.POINT_HIT_DTYPE)
            rec["prim"] = native.NO_PRIM
            if k:
                rec["prim"][:, :2] = [0, 3]
            else:
                rec["prim"][:] = 1
            return rec

    r = RVPT(8, 8)
    r._ctx, r._device_built, r._n_triangles = Recorder(), False, 4
    r.primitive_indices = np.array([2, 0, 3, 1], dtype=np.uint32)  # stored row s is added triangle primitive_indices[s]
    out = r.closest_points(np.zeros((2, 3)), k=3)
    assert r._ctx.k == 3 and out.shape == (2, 3) and out["prim"].tolist() == [[2, 1, native.NO_PRIM]] * 2
    out = r.closest_points(np.zeros((2, 3)))
    assert r._ctx.k is None and out.shape == (2,) and out["prim"].tolist() == [0, 0]
    assert "tie between equal distances is broken on the stored number, before this renumbering" in " ".join(RVPT.closest_points.__doc__.split())
