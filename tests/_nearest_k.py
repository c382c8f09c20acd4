"""The records the k-nearest point-query tests ask with (include/rvpt_hip.h: K-NEAREST POINTS).  The statement itself is rvpt_amd/scene.py: closest_points_k —
a stable sort of closest_point_triangles' candidates — and tests/test_nearest_k_host.py checks it; here are the group builder, the poison for the out fields
and for the followers' in fields, the answer as a query leaves it and the comparison."""
import numpy as np

import _nearest as nq
from rvpt_amd import native, scene

NO_PRIM = nq.NO_PRIM
POISON = 0xCDCDCDCD
IN_FIELDS, OUT_FIELDS = nq.IN_FIELDS, nq.OUT_FIELDS


def groups(points, k):
    """n * k records (flat) for the points `points` (POINT_HIT_DTYPE[n], as _nearest builds them): record 0 of a group is the point and its bound; the
    followers' in fields and every out field carry poison, so a field the library wrote, or failed to write, or read from a follower, shows"""
    out = np.empty((points.shape[0], k), dtype=native.POINT_HIT_DTYPE)
    out.view(np.uint32)[...] = POISON
    out[:, 0] = nq.poisoned(points)
    return out.reshape(-1)


def answer_k(tris, records, k):
    """`records` (n * k of them, flat or [n, k]) as a k-nearest query leaves them: scene.closest_points_k on `tris` — in the order the update form takes, the
    numbering of prim — in the out fields, every in field as it came"""
    g = records.reshape(-1, k)
    want = scene.closest_points_k(tris, g["point"][:, 0], k, g["max_d2"][:, 0])
    miss = want["prim"] == NO_PRIM
    bound_bits = np.broadcast_to(g["max_d2"][:, :1].view(np.uint32), miss.shape)  # the bits of record 0's max_d2 as given, a NaN's payload included
    want["d2"].view(np.uint32)[miss] = bound_bits[miss]
    for name in IN_FIELDS:
        want[name].view(np.uint32)[...] = g[name].view(np.uint32)
    return want.reshape(records.shape)


def check_k(got, want, records, k, what):
    got, want, records = got.reshape(-1), want.reshape(-1), records.reshape(-1)
    assert got.shape == want.shape == records.shape and got.shape[0] % k == 0
    assert nq.same_bytes(got, want), f"{what}: {nq.first_difference(got, want)}"
    for name in IN_FIELDS:  # the in fields come back byte for byte, the followers' poison included
        assert got[name].tobytes() == records[name].tobytes(), (what, name)
    g = got.reshape(-1, k)
    miss = g["prim"] == NO_PRIM
    assert (miss[:, 1:] >= miss[:, :-1]).all(), what  # from the first slot no candidate fills, every slot is a miss
    bound_bits = np.broadcast_to(records.reshape(-1, k)["max_d2"][:, :1].view(np.uint32), miss.shape)
    assert not g["closest"][miss].view(np.uint32).any() and (g["d2"].view(np.uint32)[miss] == bound_bits[miss]).all()
    assert not g["u"][miss].view(np.uint32).any() and not g["v"][miss].view(np.uint32).any() and not g["region"][miss].any()


def with_bound_variants_at(base, tris, k):
    """`base` (POINT_HIT_DTYPE[n]) followed by _nearest.with_bound_variants taken at the j-th answer's d2, for every j < k the point has: exactly it (accepted:
    the bound is not strict, so entry j and everything tied with it stay), nextafter below it (entry j is out), 0, and the other variants of _nearest"""
    full = scene.closest_points_k(tris, base["point"], k, base["max_d2"])
    out = [base]
    for j in range(k):
        column = np.ascontiguousarray(full[:, j])
        out.append(nq.with_bound_variants(base, column)[base.shape[0]:])
    return np.concatenate(out)


def point_set_k(tris, seed, k, counts=(300, 120, 120, 120, 60), variants_of=40):
    """(records, want) for one k: base_points, the bound variants at the j-th answer of the first `variants_of` of them, thirteen non-finite records; grouped
    and poisoned; and the statement's answer"""
    base = nq.base_points(tris, seed, counts)
    with np.errstate(all="ignore"):
        points = np.concatenate([base, with_bound_variants_at(base[:variants_of], tris, k)[variants_of:], nq.non_finite_records(base, seed + 1, 13)])
        records = groups(points, k)
        want = answer_k(tris, records, k)
    records.setflags(write=False)
    want.setflags(write=False)
    return records, want


def diagonal_points(zs):
    """Points on the shared diagonal x == y of _multi_hit.layered_scene's quads, an eighth in front of every layer that has an exact duplicate: the two
    triangles of a quad are equally far (dyadic coordinates: the edge's quotient is exact), and so are the duplicate's two — four candidates at one d2"""
    pts = [(x, x, z - 0.125) for z in sorted(set(np.asarray(zs)[np.asarray([np.sum(zs == z) == 4 for z in zs])].tolist())) for x in (-0.5, -0.25, 0.125, 0.25, 0.5)]
    return nq.make_records(np.asarray(pts, np.float32))
