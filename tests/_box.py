"""The records the box-query tests ask with (include/rvpt_hip.h: BOX OVERLAPS).  The statement itself is rvpt_amd/scene.py: triangle_box_overlaps / box_overlaps
and tests/test_box_host.py checks it — against an exact rational separating-axis test among others, which lives here too; here are the box generator, the group
builder with its poison, the answer as a query leaves it and the comparison."""
from fractions import Fraction

import numpy as np

from rvpt_amd import native, scene

NO_PRIM = 0xFFFFFFFF
POISON = 0xCDCDCDCD
KS = (1, 2, 3, 4)


def slots(k):
    return 4 * k - 1


def _vertices(tris):
    return np.asarray(tris, np.float32).reshape(-1, 4, 4)[:, :3, :3]


def boxes_of(tris, seed, n_surface=1100, n_off=520, n_far=90, n_flat=120, n_invalid=42, n_paged=150):
    """(lo, hi, prim_from, flags) for about 2 000 boxes against `tris`, shuffled so that a wave holds every kind:
    n_surface centred on points of the surface (random barycentrics of random triangles), n_off centred uniformly in 1.5x the scene's box, n_far centred 8 to
    128 extents away — each with its own edge per axis, log-uniform from 1/64 of the extent to twice the extent;
    n_flat degenerate boxes: lo == hi on a vertex, on a surface point, and plane probes (one axis of zero thickness through a vertex);
    n_invalid invalid ones: a NaN, +inf or -inf in one corner component, lo above hi on one axis, lo = -inf with hi = +inf;
    n_paged copies of earlier boxes with prim_from drawn from 1 .. n_tris + 7, a few at 0xFFFFFFFF.  flags carry noise: they are ignored."""
    rng = np.random.RandomState(seed)
    v = _vertices(tris)
    flat = v.reshape(-1, 3).astype(np.float64)
    blo, bhi = flat.min(axis=0), flat.max(axis=0)
    centre, ext = (blo + bhi) / 2, float((bhi - blo).max())

    def surface(n):
        w = rng.dirichlet((1.0, 1.0, 1.0), n)
        return (v[rng.randint(0, v.shape[0], n)].astype(np.float64) * w[:, :, None]).sum(axis=1)

    def sized(c):
        half = 0.5 * ext * 2.0 ** rng.uniform(-6.0, 1.0, c.shape)
        return c - half, c + half

    d = rng.normal(size=(n_far, 3))
    far = centre + ext * 2.0 ** rng.uniform(3.0, 7.0, (n_far, 1)) * d / np.linalg.norm(d, axis=1, keepdims=True)
    lo, hi = [np.concatenate(p) for p in zip(sized(surface(n_surface)), sized(centre + (bhi - blo) * rng.uniform(-0.75, 0.75, (n_off, 3))), sized(far))]
    third = n_flat // 3
    on_vertex = flat[rng.randint(0, flat.shape[0], third)]
    on_surface = surface(third).astype(np.float32).astype(np.float64)
    plane_lo, plane_hi = sized(flat[rng.randint(0, flat.shape[0], n_flat - 2 * third)])
    axis = rng.randint(0, 3, plane_lo.shape[0])
    through = 0.5 * (plane_lo + plane_hi)  # the vertex again
    rows = np.arange(plane_lo.shape[0])
    plane_lo[rows, axis] = plane_hi[rows, axis] = through[rows, axis]
    lo = np.concatenate([lo, on_vertex, on_surface, plane_lo]).astype(np.float32)
    hi = np.concatenate([hi, on_vertex, on_surface, plane_hi]).astype(np.float32)
    assert (lo <= hi).all()
    n_valid = lo.shape[0]
    # invalid records, made from valid ones
    src = rng.randint(0, n_valid, n_invalid)
    bad_lo, bad_hi = lo[src].copy(), hi[src].copy()
    for i in range(n_invalid):
        a, kind = rng.randint(0, 3), i % 6
        if kind < 3:
            (bad_lo if rng.rand() < 0.5 else bad_hi)[i, a] = (np.nan, np.inf, -np.inf)[kind]
        elif kind < 5:
            bad_lo[i, a], bad_hi[i, a] = bad_hi[i, a] + np.float32(ext / 64), bad_lo[i, a]  # lo above hi on one axis
        else:
            bad_lo[i, a], bad_hi[i, a] = -np.inf, np.inf  # ordered, and still not finite
    src = rng.randint(0, n_valid, n_paged)
    first = rng.randint(1, v.shape[0] + 8, n_paged).astype(np.uint32)
    first[::29] = NO_PRIM
    lo, hi = np.concatenate([lo, bad_lo, lo[src]]), np.concatenate([hi, bad_hi, hi[src]])
    prim_from = np.concatenate([np.zeros(n_valid + n_invalid, np.uint32), first])
    order = rng.permutation(lo.shape[0])
    flags = rng.randint(0, 2 ** 32, lo.shape[0], dtype=np.uint64).astype(np.uint32)
    return lo[order], hi[order], prim_from[order], flags


def groups(lo, hi, prim_from=0, flags=0, k=1):
    """n * k records (flat): record 0 of a group carries the box; the followers' in quads and every out quad carry poison, so a word the library wrote, or
    failed to write, or read from a follower, shows"""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    out = np.empty((lo.shape[0], k), dtype=native.BOX_OVERLAP_DTYPE)
    out.view(np.uint32)[...] = POISON
    head = np.empty(lo.shape[0], dtype=native.BOX_OVERLAP_DTYPE)
    head.view(np.uint32)[...] = POISON
    head["lo"], head["hi"], head["prim_from"], head["flags"] = lo, np.asarray(hi, np.float32).reshape(-1, 3), prim_from, flags
    out[:, 0] = head
    return out.reshape(-1)


def answer(tris, records, k, perm=None):
    """`records` as a box query leaves them: scene.box_overlaps on `tris` (in the order the update form takes, the numbering of prim), every in quad as it came"""
    assert scene.BOX_OVERLAP_DTYPE == native.BOX_OVERLAP_DTYPE
    with np.errstate(all="ignore"):
        return scene.box_overlaps(tris, records, k, perm)


def lists(records, k):
    """(count[n], numbers[n, 4k - 1])"""
    return native.box_overlap_lists(records, k)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def first_difference(got, want, k):
    g, w = np.ascontiguousarray(got).reshape(-1).view(np.uint32).reshape(-1, 12), np.ascontiguousarray(want).reshape(-1).view(np.uint32).reshape(-1, 12)
    bad = np.flatnonzero((g != w).any(axis=1))
    i = int(bad[0])
    grp = i // k
    return (f"{bad.size} of {g.shape[0]} records differ; first: record {i} (group {grp}, record {i % k} of it): got {g[i].tolist()}, want {w[i].tolist()}; "
            f"the group's box: {np.ascontiguousarray(want).reshape(-1)[grp * k]}")


def check(got, want, records, k, what):
    got, want, records = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1), np.ascontiguousarray(records).reshape(-1)
    assert got.shape == want.shape == records.shape and got.shape[0] % k == 0
    assert same_bytes(got, want), f"{what}: {first_difference(got, want, k)}"
    words, given = got.view(np.uint32).reshape(-1, 12), records.view(np.uint32).reshape(-1, 12)
    assert (words[:, :8] == given[:, :8]).all(), what  # the in quads come back byte for byte, the followers' poison included
    count, numbers = lists(got, k)
    filled = numbers != NO_PRIM
    assert (filled[:, 1:] <= filled[:, :-1]).all(), what  # from the first slot A does not fill, every slot is 0xFFFFFFFF
    assert (filled.sum(axis=1) == np.minimum(count, slots(k))).all(), what
    assert (np.diff(numbers.astype(np.int64), axis=1)[filled[:, 1:]] > 0).all(), what  # ascending


def box_set(tris, seed, k, **counts):
    """(records, want) for one k on `tris`: boxes_of's boxes grouped and poisoned, and the statement's answer; read-only"""
    lo, hi, prim_from, flags = boxes_of(tris, seed, **counts)
    records = groups(lo, hi, prim_from, flags, k)
    want = answer(tris, records, k)
    records.setflags(write=False)
    want.setflags(write=False)
    return records, want


def census(want, k):
    """how the groups of an answered set fall: (count == 0 and valid or not, 0 < count <= S, count > S, invalid, groups)"""
    g = np.ascontiguousarray(want).reshape(-1, k)
    lo, hi = g["lo"][:, 0], g["hi"][:, 0]
    with np.errstate(all="ignore"):
        invalid = ~(np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1))
    count = g["count"][:, 0]
    return int((count == 0).sum()), int(((count > 0) & (count <= slots(k))).sum()), int((count > slots(k)).sum()), int(invalid.sum()), g.shape[0]


def exact_overlap(a, b, c, lo, hi) -> bool:
    """The separating-axis test of the triangle (a, b, c) against the closed box [lo, hi] in exact rational arithmetic: the same 13 axes as THE TEST — the box's
    three, the triangle's normal, the nine cross products of an edge with an axis — with no rounding anywhere.  Separated iff, on some axis, the triangle's
    interval and the box's do not touch.  Arguments are sequences of three ints or Fractions each."""
    a, b, c = ([Fraction(x) for x in p] for p in (a, b, c))
    lo, hi = [Fraction(x) for x in lo], [Fraction(x) for x in hi]
    ctr = [(l + h) / 2 for l, h in zip(lo, hi)]
    half = [h - m for h, m in zip(hi, ctr)]
    v = [[p[i] - ctr[i] for i in range(3)] for p in (a, b, c)]
    e = [[b[i] - a[i] for i in range(3)], [c[i] - b[i] for i in range(3)], [a[i] - c[i] for i in range(3)]]

    def cross(x, y):
        return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]

    unit = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    axes = unit + [cross(e[0], [c[i] - a[i] for i in range(3)])] + [cross(ei, u) for ei in e for u in unit]
    for ax in axes:
        p = [sum(ax[i] * vm[i] for i in range(3)) for vm in v]
        r = sum(abs(ax[i]) * half[i] for i in range(3))
        if min(p) > r or max(p) < -r:
            return False
    return True
