"""Point queries without a GPU: the record of include/rvpt_hip.h is the record of rvpt_amd/native.py; the numpy statement (rvpt_amd/scene.py:
closest_point_triangles / closest_points) computes what the header specifies, unfused, in the specified region order; the clamp and the box inequality that
make pruning exact hold; the statement agrees with a float64 restatement; the wrappers refuse what they can see to be wrong before any call."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _nearest as nq

ROOT = Path(__file__).resolve().parent.parent
OFFSETS = {"point": 0, "max_d2": 12, "closest": 16, "d2": 28, "prim": 32, "u": 36, "v": 40, "region": 44}
F = np.float32
EPS32 = 2.0 ** -23


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def b1(x) -> int:
    return int(np.asarray(x, dtype=np.float32).reshape(-1)[0].view(np.uint32))


def test_the_header_record_compiles_as_c99_with_the_pinned_layout(tmp_path):
    fields = ", ".join(f"offsetof(rvpt_point_hit, {f})" for f in OFFSETS)
    src = ('#include "rvpt_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu ' + " ".join(["%zu"] * len(OFFSETS)) + ' %d\\n", sizeof(rvpt_point_hit), '
           + fields + ", RVPT_HIP_FORMAT_NEAREST_POINTS);return 0;}\n")
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [48, *OFFSETS.values(), 4]


def test_the_bindings_record_is_the_headers():
    from rvpt_amd import native, scene
    assert native.POINT_HIT_DTYPE.itemsize == 48 and scene.POINT_HIT_DTYPE == native.POINT_HIT_DTYPE
    assert {n: native.POINT_HIT_DTYPE.fields[n][1] for n in native.POINT_HIT_DTYPE.names} == OFFSETS
    text = (ROOT / "include" / "rvpt_hip.h").read_text()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (RVPT_HIP_[A-Z0-9_]+) (0x[0-9A-Fa-f]+|\d+)u?\b", text)}
    assert defs["RVPT_HIP_FORMAT_NEAREST_POINTS"] == native.FORMAT_NEAREST_POINTS == 4
    assert defs["RVPT_HIP_ABI_VERSION"] == native.ABI_VERSION == 8 and "new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_NEAREST_POINTS (4)" in text
    kernel_side = (ROOT / "rvpt_amd" / "csrc" / "rvpt_nearest.h").read_text()
    assert int(re.search(r"constexpr uint32_t kNearestRecordBytes = (\d+);", kernel_side).group(1)) == 48
    assert scene.NO_PRIM == native.NO_PRIM == nq.NO_PRIM


def scalar_candidate(a, b, c, p, fused=False):
    """The header's arithmetic for ONE triangle and point in np.float32 scalars, as a chain of ifs.  fused: the same with every `x*y + z` of the dots and of q
    contracted (the product kept exact in float64, one rounding) — what a compiler that fuses would compute."""
    a, b, c, p = (np.asarray(x, F) for x in (a, b, c, p))

    def mad(x, y, z):  # x*y + z
        return F(np.float64(x) * np.float64(y) + np.float64(z)) if fused else F(F(x * y) + z)

    def dot(x, y):
        return mad(x[2], y[2], mad(x[1], y[1], F(x[0] * y[0])))

    def quot(n, d):
        return F(0) if d == 0 else F(n / d)

    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = F(d1 * d4) - F(d3 * d2), F(d5 * d2) - F(d1 * d6), F(d3 * d6) - F(d5 * d4)
        e1, e2 = d4 - d3, d5 - d6
        if d1 <= 0 and d2 <= 0:
            u, v, region = F(0), F(0), 1
        elif d3 >= 0 and d4 <= d3:
            u, v, region = F(1), F(0), 2
        elif vc <= 0 and d1 >= 0 and d3 <= 0:
            u, v, region = quot(d1, d1 - d3), F(0), 4
        elif d6 >= 0 and d5 <= d6:
            u, v, region = F(0), F(1), 3
        elif vb <= 0 and d2 >= 0 and d6 <= 0:
            u, v, region = F(0), quot(d2, d2 - d6), 5
        elif va <= 0 and e1 >= 0 and e2 >= 0:
            w = quot(e1, e1 + e2)
            u, v, region = F(1) - w, w, 6
        else:
            s = F(va + vb) + vc
            u, v, region = quot(vb, s), quot(vc, s), 0
        q = np.array([mad(ac[i], v, mad(ab[i], u, a[i])) for i in range(3)], F)
        lo, hi = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
        q = np.array([lo[i] if q[i] < lo[i] else (hi[i] if q[i] > hi[i] else q[i]) for i in range(3)], F)
        d = p - q
        dist2 = F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2])
    return q, F(dist2), F(u), F(v), region


def test_the_arithmetic_is_unfused_and_takes_the_first_region_that_holds():
    """600 random triangle/point pairs: the vectorised statement equals the scalar chain of ifs bit for bit in every field; a fused evaluation of the dots and of
    q changes bits of u, v, closest or d2 in many of them, so the comparison does tell the two apart."""
    from rvpt_amd import scene
    rng = np.random.RandomState(1)
    fused_differs = 0
    seen = set()
    for k in range(600):
        a, b, c = (rng.uniform(-1, 1, 3).astype(F) for _ in range(3))
        p = rng.uniform(-1.5, 1.5, 3).astype(F)
        tri = np.zeros((1, 16), F)
        tri.reshape(4, 4)[:3, :3] = (a, b, c)
        q, d2, u, v, region = scene.closest_point_triangles(p, tri)
        got = (bits(q[0]).tolist(), b1(d2), b1(u), b1(v), int(region[0]))
        plain = scalar_candidate(a, b, c, p)
        assert got == (bits(plain[0]).tolist(), b1(plain[1]), b1(plain[2]), b1(plain[3]), plain[4]), k
        fused = scalar_candidate(a, b, c, p, fused=True)
        fused_differs += got != (bits(fused[0]).tolist(), b1(fused[1]), b1(fused[2]), b1(fused[3]), fused[4])
        seen.add(int(region[0]))
    assert seen == set(range(7)) and fused_differs > 100, (seen, fused_differs)
    # ... and one pair by hand where fusing the dot changes it: ab = (1, x, 0), ap = (-1, x, 0) with x = 1 + 2^-12: the unfused d1 is
    # RN(-1 + RN(x^2)) = 2^-11 (the 2^-24 of the square is rounded away first), the fused one 2^-11 + 2^-24; d3 = -2, so the edge ab decides: u = d1 / (d1 + 2)
    x = F(1 + 2.0 ** -12)
    a, b, c, p = np.zeros(3, F), np.array([1, x, 0], F), np.array([0, 0, 1], F), np.array([-1, x, 0], F)
    plain, fused = scalar_candidate(a, b, c, p), scalar_candidate(a, b, c, p, fused=True)
    assert plain[4] == fused[4] == 4 and b1(plain[2]) == b1(F(2.0 ** -11) / F(2 + 2.0 ** -11)) != b1(fused[2])
    tri = np.zeros((1, 16), F)
    tri.reshape(4, 4)[:3, :3] = (a, b, c)
    got = scene.closest_point_triangles(p, tri)
    assert b1(got[2]) == b1(plain[2]) and bits(got[0][0]).tolist() == bits(plain[0]).tolist() != bits(fused[0]).tolist()


@pytest.fixture(scope="module")
def default_set():
    from rvpt_amd import scene
    tris, _ = scene.default_scene()
    return (tris, *nq.point_set(tris, 3))


def test_the_generator_reaches_every_region_and_every_kind_of_record(default_set):
    tris, records, want = default_set
    hit = want["prim"] != nq.NO_PRIM
    assert set(np.unique(want["region"][hit]).tolist()) == set(range(7))
    assert hit.sum() > 1000 and (~hit).sum() > 1000
    assert (want["prim"][-12:] == nq.NO_PRIM).all()  # the non-finite points
    with np.errstate(all="ignore"):
        assert (want["prim"][records["max_d2"] < 0] == nq.NO_PRIM).all() and (want["prim"][np.isnan(records["max_d2"])] == nq.NO_PRIM).all()
    neg_zero = bits(records["max_d2"]) == 0x80000000
    assert neg_zero.any() and (want["prim"][neg_zero] != nq.NO_PRIM).any()  # -0.0 is a valid bound: points on the surface are found
    assert (want["d2"][neg_zero & hit] == 0).all()
    assert bits(want["d2"][~hit]).tolist() == bits(records["max_d2"][~hit]).tolist()
    # d2 == max_d2 is accepted, nextafter(d2, 0) is not (unless another triangle sits at that very distance, which it then reports)
    base = np.flatnonzero(np.isinf(records["max_d2"]) & hit & (want["d2"] > 0))
    n_base = int(np.isinf(records["max_d2"]).sum())
    n_hit = int((np.isinf(records["max_d2"]) & hit).sum())
    exact = records["max_d2"][n_base + n_hit:n_base + 2 * n_hit]
    assert bits(want["d2"][n_base + n_hit:n_base + 2 * n_hit]).tolist() == bits(exact).tolist() and base.size > 500


def test_the_clamp_keeps_closest_inside_the_triangles_box(default_set):
    tris, records, want = default_set
    hit = want["prim"] != nq.NO_PRIM
    v = tris.reshape(-1, 4, 4)[:, :3, :3][want["prim"][hit]]
    q = want["closest"][hit]
    assert (q >= v.min(axis=1)).all() and (q <= v.max(axis=1)).all()
    # every candidate of every triangle too, not only the winners
    q_all = np.concatenate([__import__("rvpt_amd.scene", fromlist=["x"]).closest_point_triangles(records["point"][:-12][k::7][:300], tris)[0] for k in range(2)])
    va = tris.reshape(-1, 4, 4)[:, :3, :3]
    assert (q_all >= va.min(axis=1)).all() and (q_all <= va.max(axis=1)).all()


def test_zero_divisors_and_zero_area_triangles_give_finite_bytes():
    from rvpt_amd import scene
    a, b, c = np.array([0.25, 0.5, -1], F), np.array([1.5, 0.5, 2], F), np.array([-0.75, 2, 0.5], F)
    cases = {"a==b": (a, a, c), "b==c": (a, b, b), "a==c": (a, b, a), "a==b==c": (a, a, a), "collinear": (a, (a + b) / F(2), b)}
    pts = np.array([[0, 0, 0], [0.25, 0.5, -1], [3, -2, 5], [0.875, 0.5, 0.5], [-4, 7, 0.25]], F)
    for name, (x, y, z) in cases.items():
        tri = np.zeros((1, 16), F)
        tri.reshape(4, 4)[:3, :3] = (x, y, z)
        q, d2, u, v, region = scene.closest_point_triangles(pts, tri)
        assert np.isfinite(q).all() and np.isfinite(d2).all() and np.isfinite(u).all() and np.isfinite(v).all(), name
        lo, hi = np.minimum(np.minimum(x, y), z), np.maximum(np.maximum(x, y), z)
        assert (q >= lo).all() and (q <= hi).all(), name
        # a point of its box, its error bounded by the triangle's own extent: no farther than the nearest vertex plus the box's diagonal
        near = np.sqrt(((pts[:, None, :].astype(np.float64) - np.array([x, y, z], np.float64)) ** 2).sum(axis=2)).min(axis=1)
        assert (np.sqrt(d2[:, 0].astype(np.float64)) <= near + np.linalg.norm((hi - lo).astype(np.float64)) + 1e-6).all(), name
    tri = np.zeros((1, 16), F)
    tri.reshape(4, 4)[:3, :3] = (a, a, c)
    q, d2, u, v, region = scene.closest_point_triangles(np.array([1, 1, 1], F), tri)
    assert region[0] in (1, 4) and bits(q[0]).tolist() == bits(a).tolist()  # with a == b the edge-ab region (or a's own) answers a
    rec = scene.closest_points(tri, pts)
    assert (rec["prim"] == 0).all() and np.isfinite(rec["d2"]).all()


def _trees(tris, which):
    from rvpt_amd import scene
    nodes, perm = {"sah": scene.build_sah, "lbvh": scene.build_lbvh}[which if which != "grown" else "sah"](tris)[:2]
    if which == "grown":
        nodes = nq.grown_boxes(nodes, 4)
    return np.ascontiguousarray(nodes).view(__import__("rvpt_amd.native", fromlist=["x"]).NODE_DTYPE).reshape(-1), tris[perm]


@pytest.mark.parametrize("which", ["sah", "lbvh", "grown"])
@pytest.mark.parametrize("name", ["default", "cornell"])
def test_the_box_inequality_holds_for_every_node(name, which):
    """box_d2(node) <= d2_i in float32 for every node of the tree and EVERY triangle under it, for 56 points of every kind: what lets a walk skip a node iff
    box_d2 > best and still return the brute-force answer."""
    from rvpt_amd import scene
    tris = scene.default_scene()[0] if name == "default" else scene.cornell_scene(2)[0]
    assert tris.shape[0] == (143 if name == "default" else 2300)
    nodes, stored = _trees(tris, which)
    pts = nq.base_points(stored, 5, counts=(16, 6, 6, 4, 2))["point"]
    assert pts.shape[0] == 56
    d2 = scene.closest_point_triangles(pts, stored)[1]  # [56, n]
    under = nq.triangles_under(nodes)
    assert len(under) >= 2 * (tris.shape[0] // 8) and under[0].shape[0] == tris.shape[0]
    v = stored.reshape(-1, 4, 4)[:, :3, :3]
    strict = 0
    for i, idx in under.items():
        lo, hi = nodes["bounds"][i][0::2], nodes["bounds"][i][1::2]
        assert (v[idx].min(axis=(0, 1)) >= lo).all() and (v[idx].max(axis=(0, 1)) <= hi).all()  # the premise: a box contains its vertices
        box = scene.point_box_d2(pts, lo, hi)  # [56]
        assert (box[:, None] <= d2[:, idx]).all(), (i, which)
        strict += int((box > 0).sum())
    assert strict > len(under)  # (the inequality was not 0 <= d2 throughout)


def _distance64(p, a, b, c):
    """Ericson's test in float64 (the regions by the same predicates): the distance from p to the triangle, and the region"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c

    def dot(x, y):
        return (x * y).sum(axis=-1)

    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)]
    region = np.select(conds, [1, 2, 4, 3, 5, 6], default=0)
    s = va + vb + vc
    with np.errstate(all="ignore"):
        w = e1 / (e1 + e2)
        u = np.select([region == 2, region == 4, region == 6, region == 0], [np.ones_like(s), d1 / (d1 - d3), 1 - w, vb / s], default=0.0)
        v = np.select([region == 3, region == 5, region == 6, region == 0], [np.ones_like(s), d2 / (d2 - d6), w, vc / s], default=0.0)
    q = a + ab * u[:, None] + ac * v[:, None]
    return np.linalg.norm(p - q, axis=1), region


@pytest.mark.parametrize("name", ["default", "cornell"])
def test_the_statement_agrees_with_a_float64_restatement(name):
    """sqrt(d2) of every answered record against the float64 distance from the point to the SAME triangle (prim), within a bound derived from the operation
    count, in units of eps = 2^-23 times M, the largest coordinate magnitude among a, b, c and p (differences of coordinates are below 2 M, distances below
    2 sqrt(3) M); unit roundoff is eps / 2.
      (1) d2 from p and the stored q: three differences, three squares, two sums — five roundings on the way to each term, relative error of d2 below
          5 eps / 2, of its root below 5 eps / 4: at most 1.25 * 2 sqrt(3) = 4.4 eps M.
      (2) q from (u, v): ab, ac (one rounding each, 2 M eps / 2), the two products and the two sums (each on values below 3 M): per component at most
          (1 + 1 + 1.5) * 2 = 7 eps M, as a length 7 sqrt(3) = 12.2 eps M from the point Q(u, v) of the triangle's plane; the clamp moves q towards the box only.
      (3) (u, v) of a vertex or edge region: a dot has two operand roundings and three of its own, |error| <= 5 (eps / 2) |x| |y|; u = d1 / (d1 - d3) moves
          Q by |ab| du <= 2 * 2.5 eps * 2 sqrt(3) M = 17.4 eps M along the edge (numerator and denominator).
      Together 34 eps M; asserted at 40.  Q lies in the triangle, so the true distance is never larger than |p - Q|: the LOWER side has (1) + (2) only.
      (4) the face region's (u, v) = (vb, vc) / s carry the cancellation of vb = d5 d2' - d1 d6: the lateral error is at most
          delta = 96 eps D'^2 / (h sin^2) — D' the largest of |ap|, |bp|, |cp|, h the shorter of |ab|, |ac|, sin^2 = |ab x ac|^2 / (|ab|^2 |ac|^2): 12 roundings per
          product of dots, two products and the difference, s three times that — but p - q* is perpendicular to the face, so delta enters the distance in second
          order only: min(delta, diagonal)^2 / (2 D), and never more than min(delta, diagonal) (the clamp).  That term is computed per record in float64 and added
          to the upper side.
    Zero-area triangles have no sin^2: they are excluded by the explicit area test |ab x ac| >= 2^-20 |ab| |ac|, and the excluded share is asserted to be 0 on
    these two scenes.  Measured when this was written: between -0.7 and +1.0 eps M on both scenes."""
    from rvpt_amd import scene
    tris = scene.default_scene()[0] if name == "default" else scene.cornell_scene(2)[0]
    records, want = nq.point_set(tris, 3, counts=(300, 120, 120, 120, 60) if name == "default" else (200, 60, 60, 60, 30))
    hit = want["prim"] != nq.NO_PRIM
    assert hit.sum() > 500
    t = tris.reshape(-1, 4, 4)[:, :3, :3][want["prim"][hit]].astype(np.float64)
    p = want["point"][hit].astype(np.float64)
    ab, ac = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    cross = np.linalg.norm(np.cross(ab, ac), axis=1)
    lab, lac = np.linalg.norm(ab, axis=1), np.linalg.norm(ac, axis=1)
    keep = cross >= 2.0 ** -20 * lab * lac
    assert (~keep).sum() == 0
    d64, region64 = _distance64(p, t[:, 0], t[:, 1], t[:, 2])
    d32 = np.sqrt(want["d2"][hit].astype(np.float64))
    M = np.maximum(np.abs(t).reshape(t.shape[0], -1).max(axis=1), np.abs(p).max(axis=1))
    reach = np.linalg.norm(p[:, None, :] - t, axis=2).max(axis=1)
    delta = 96 * EPS32 * reach ** 2 / (np.minimum(lab, lac) * (cross / (lab * lac)) ** 2)
    delta = np.minimum(delta, np.linalg.norm(t.max(axis=1) - t.min(axis=1), axis=1))
    with np.errstate(all="ignore"):
        second = np.minimum(delta, np.where(d64 > 0, delta ** 2 / (2 * d64), delta))
    err = d32 - d64
    print(f"{name}: {hit.sum()} answered, error {err.min() / (EPS32 * M[err.argmin()]):.2f} .. {err.max() / (EPS32 * M[err.argmax()]):.2f} eps M, regions {np.bincount(region64, minlength=7).tolist()}")
    assert (err >= -17 * EPS32 * M).all() and (err <= 40 * EPS32 * M + second).all()
    assert (np.bincount(region64, minlength=7) > 0).all()


def test_ties_go_to_the_smaller_index():
    """duplicated triangles: equal d2, the smaller index wins, whatever the order of the array; a bound below the distance finds neither"""
    from rvpt_amd import scene
    tris, _ = scene.default_scene()
    dup = np.concatenate([tris[:40], tris[:40][::-1], tris[10:20]])
    pts = nq.base_points(tris[:40], 9, counts=(100, 30, 30, 30, 10))["point"]
    rec = scene.closest_points(dup, pts)
    assert (rec["prim"] < 40).all()
    first = scene.closest_points(tris[:40], pts)
    assert rec.tobytes() == first.tobytes()
    rev = scene.closest_points(dup[::-1].copy(), pts)  # the same triangles, numbered backwards: the same distances, other winners
    assert bits(rev["d2"]).tolist() == bits(rec["d2"]).tolist() and (rev["prim"] != rec["prim"]).any()
    d2 = scene.closest_point_triangles(pts, dup[::-1].copy())[1]
    k = np.arange(pts.shape[0])
    assert (rev["prim"] == np.argmax(d2 == d2[k, rev["prim"]][:, None], axis=1)).all()
    # shared vertices and edges of the mesh itself tie too: among the triangles at the winning distance the reported one is the first
    on_vertex = scene.closest_points(tris, tris.reshape(-1, 4, 4)[:, 0, :3])
    d2 = scene.closest_point_triangles(on_vertex["point"], tris)[1]
    assert (on_vertex["d2"] == 0).all() and (on_vertex["prim"] == np.argmax(d2 == 0, axis=1)).all() and ((d2 == 0).sum(axis=1) > 1).any()
    # a NaN candidate never wins, not even against nothing
    bad = tris[:3].copy()
    bad[1, 0] = np.nan
    rec = scene.closest_points(bad, pts[:50])
    assert (rec["prim"] != 1).all() and (rec["prim"] != nq.NO_PRIM).all()
    assert (scene.closest_points(bad[1:2], pts[:50])["prim"] == nq.NO_PRIM).all()


class _Recorder:
    """stands in for the library: records what reaches rvpt_hip_read"""

    def __init__(self):
        self.calls = []

    def rvpt_hip_read(self, handle, fmt, ptr, nbytes):
        import ctypes
        self.calls.append((handle, fmt, ctypes.cast(ptr, ctypes.c_void_p).value, nbytes))
        return 0


HANDLE = __import__("ctypes").c_void_p(0)  # (a null handle: Context.close has nothing to destroy)


def _context(lib=None):
    from rvpt_amd import native
    ctx = object.__new__(native.Context)
    ctx._L, ctx._h = lib, (None if lib is None else HANDLE)
    ctx.device = 0
    return ctx


def test_closest_points_into_reaches_the_library_with_format_4():
    import torch
    from rvpt_amd import native
    lib = _Recorder()
    ctx = _context(lib)
    rec = np.zeros(5, dtype=native.POINT_HIT_DTYPE)
    assert ctx.closest_points_into(rec) is rec
    t = torch.zeros((7, 12), dtype=torch.float32)
    assert ctx.closest_points_into(t) is t
    assert lib.calls == [(HANDLE, 4, rec.ctypes.data, 240), (HANDLE, 4, t.data_ptr(), 336)]
    out = ctx.closest_points([[0, 1, 2], [3, 4, 5]], max_dist=[1.5, np.inf])
    assert out.dtype == native.POINT_HIT_DTYPE and lib.calls[-1][1:] == (4, out.ctypes.data, 96)
    assert out["point"].tolist() == [[0, 1, 2], [3, 4, 5]] and out["max_d2"].tolist() == [2.25, np.inf]  # the distance squared in float32
    x = np.float32(1.1)
    assert bits(ctx.closest_points([0, 0, 0], x)["max_d2"])[0] == bits(x * x)
    assert ctx.closest_points(np.zeros((3, 3)))["max_d2"].tolist() == [np.inf] * 3
    assert ctx.closest_points([0, 0, 0], -2.0)["max_d2"][0] < 0 and np.isnan(ctx.closest_points([0, 0, 0], np.nan)["max_d2"][0])  # invalid stays invalid
    assert ctx.closest_points(np.zeros((0, 3))).shape == (0,)


def test_the_wrappers_refuse_before_any_call():
    import torch
    from rvpt_amd import RVPT, native
    ctx = _context()
    good = np.zeros(4, dtype=native.POINT_HIT_DTYPE)
    with pytest.raises(AttributeError):  # (the helper's premise: a well-formed array does reach the call)
        ctx.closest_points_into(good)
    refused = [
        np.zeros(4, dtype=native.RAY_HIT_DTYPE),  # the ray queries' record
        np.zeros((4, 12), dtype=np.float32),
        np.zeros(8, dtype=native.POINT_HIT_DTYPE)[::2],  # not contiguous
        torch.zeros((4, 12), dtype=torch.float64),
        torch.zeros((4, 11), dtype=torch.float32),
        torch.zeros((4, 24), dtype=torch.float32)[:, ::2],  # not contiguous
        [0.0] * 12,
    ]
    for records in refused:
        with pytest.raises(native.NativeError) as e:
            ctx.closest_points_into(records)
        assert e.value.code == native.ERR_INVALID and "closest_points_into" in str(e.value)
    read_only = good.copy()
    read_only.setflags(write=False)
    with pytest.raises(native.NativeError, match="writeable POINT_HIT_DTYPE"):
        ctx.closest_points_into(read_only)
    for bad in (np.zeros((4, 12), dtype=np.float32), torch.zeros((4, 11), dtype=torch.float32), "records"):  # the same refusals, in the same words, as trace_rays_into
        said = []
        for call, dtype_name in ((ctx.trace_rays_into, "RAY_HIT_DTYPE"), (ctx.closest_points_into, "POINT_HIT_DTYPE")):
            with pytest.raises(native.NativeError) as e:
                call(bad)
            said.append(str(e.value).replace(call.__name__, "X").replace(dtype_name, "D"))
        assert said[0] == said[1]
    with pytest.raises(native.NativeError, match=r"points\[n, 3\] are needed"):
        ctx.closest_points(np.zeros((5, 2), np.float32))
    with pytest.raises(native.NativeError, match=r"points\[n, 3\] are needed"):
        ctx.closest_points(np.zeros(4, np.float32))
    with pytest.raises(native.NativeError, match="5 points, max_dist of shape"):
        ctx.closest_points(np.zeros((5, 3), np.float32), np.ones(4))
    # format 4 is a format of records, not of a frame: the frame wrappers go on refusing it
    with pytest.raises(native.NativeError, match="unknown format 4"):
        ctx._frame_buffer(np.zeros((2, 2, 4), np.float32), native.FORMAT_NEAREST_POINTS, "read_into")
    with pytest.raises(RuntimeError, match="closest_points before initialize"):
        RVPT(8, 8).closest_points([0, 0, 0])
