"""The points the point-query tests ask with (include/rvpt_hip.h: NEAREST POINTS).  The statement itself is rvpt_amd/scene.py: closest_points — brute force over
closest_point_triangles — and tests/test_nearest_host.py checks it; here are the record builder, the poison for the out fields and the generator."""
import numpy as np

from _ray_query import first_difference, same_bytes, shared_edge_midpoints  # noqa: F401  (what the ray queries' helpers already offer)
from rvpt_amd import native, scene

NO_PRIM = 0xFFFFFFFF
IN_FIELDS = ("point", "max_d2")
OUT_FIELDS = ("closest", "d2", "prim", "u", "v", "region")


def _vertices(tris):
    return np.asarray(tris, np.float32).reshape(-1, 4, 4)[:, :3, :3]


def poisoned(records):
    """the out fields filled with a pattern no query leaves: a field the library did not write shows"""
    rec = records.copy()
    for name in OUT_FIELDS:
        rec[name].view(np.uint32)[...] = 0xCDCDCDCD
    return rec


def make_records(points, max_d2=np.inf):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    rec = np.zeros(pts.shape[0], dtype=native.POINT_HIT_DTYPE)
    rec["point"], rec["max_d2"] = pts, np.asarray(max_d2, np.float32)
    return poisoned(rec)


def answer(tris, records, perm=None):
    """`records` with the out fields as a query leaves them: scene.closest_points on `tris` — in the order the update form takes, the numbering of prim."""
    want = scene.closest_points(tris, records["point"], records["max_d2"])
    want["max_d2"].view(np.uint32)[:] = records["max_d2"].view(np.uint32)  # the bits as given, a NaN's payload included
    miss = want["prim"] == NO_PRIM
    want["d2"].view(np.uint32)[miss] = records["max_d2"].view(np.uint32)[miss]
    want["point"].view(np.uint32)[:] = records["point"].view(np.uint32)
    return want


def base_points(tris, seed, counts=(300, 120, 120, 120, 60)):
    """Points against `tris`: uniform in 3x the scene's box; exactly on mesh vertices; midpoints of shared edges; face centroids; centroids pushed +-epsilon and
    +-one extent along the normal (four per chosen face); points 128 extents away.  counts = (uniform, vertices, edges, centroids, pushed faces); 16 far points.
    Shuffled, so that a wave holds every kind."""
    rng = np.random.RandomState(seed)
    v = _vertices(tris)
    flat = v.reshape(-1, 3)
    lo, hi = flat.min(axis=0).astype(np.float64), flat.max(axis=0).astype(np.float64)
    centre, ext = (lo + hi) / 2, float((hi - lo).max())
    n_uni, n_vert, n_edge, n_cent, n_push = counts
    pts = [centre + (hi - lo) * rng.uniform(-1.5, 1.5, (n_uni, 3))]
    pts.append(flat[rng.randint(0, flat.shape[0], n_vert)])
    mids = shared_edge_midpoints(tris)
    if mids.shape[0] == 0:
        mids = flat
    pts.append(mids[rng.randint(0, mids.shape[0], n_edge)])
    cent = ((v[:, 0] + v[:, 1]) + v[:, 2]) / np.float32(3)
    pts.append(cent[rng.randint(0, cent.shape[0], n_cent)])
    pick = rng.randint(0, cent.shape[0], n_push)
    vv = v[pick].astype(np.float64)
    nrm = np.cross(vv[:, 1] - vv[:, 0], vv[:, 2] - vv[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    for s in (1e-6 * ext, -1e-6 * ext, ext, -ext):
        pts.append(cent[pick].astype(np.float64) + s * nrm)
    d = rng.normal(size=(16, 3))
    pts.append(centre + 128.0 * ext * d / np.linalg.norm(d, axis=1, keepdims=True))
    pts = np.concatenate([np.asarray(p, np.float64) for p in pts]).astype(np.float32)
    return make_records(pts[rng.permutation(pts.shape[0])])


def with_bound_variants(records, answered):
    """`records` followed, for every record that is answered (`answered`: the statement's answer), by that point with max_d2 = d2 / 2, exactly d2 (accepted: the
    bound is not strict), nextafter(d2, 0), 0, -1, NaN and -0.0"""
    hit = np.flatnonzero(answered["prim"] != NO_PRIM)
    d2 = answered["d2"][hit]
    extra = []
    for bound in (d2 / np.float32(2), d2, np.nextafter(d2, np.float32(0)), np.zeros_like(d2), -np.ones_like(d2), np.full_like(d2, np.nan), np.full_like(d2, -0.0)):
        r = records[hit].copy()
        r["max_d2"] = bound
        extra.append(r)
    return np.concatenate([records] + extra)


def non_finite_records(records, seed, n=12):
    """n of `records` with a NaN, +inf or -inf in one component of the point"""
    rng = np.random.RandomState(seed)
    out = records[rng.randint(0, records.shape[0], n)].copy()
    for k in range(n):
        out["point"][k, rng.randint(0, 3)] = (np.nan, np.inf, -np.inf)[k % 3]
    return out


def point_set(tris, seed, counts=(300, 120, 120, 120, 60)):
    """(records, want): base_points with the bound variants of every answered one and a dozen non-finite records, poisoned; and the statement's answer"""
    base = base_points(tris, seed, counts)
    records = poisoned(np.concatenate([with_bound_variants(base, answer(tris, base)), non_finite_records(base, seed + 1, 12)]))
    want = answer(tris, records)
    records.setflags(write=False)
    want.setflags(write=False)
    return records, want


def check(got, want, records, what):
    assert same_bytes(got, want), f"{what}: {first_difference(got, want)}"
    for name in IN_FIELDS:  # the in fields come back byte for byte, NaN payloads included
        assert got[name].tobytes() == records[name].tobytes(), (what, name)
    miss = got["prim"] == NO_PRIM  # a miss's out fields are all written: closest 0, the bound's bits, u = v = 0, region 0
    assert not got["closest"][miss].view(np.uint32).any() and got["d2"][miss].tobytes() == records["max_d2"][miss].tobytes()
    assert not got["u"][miss].view(np.uint32).any() and not got["v"][miss].view(np.uint32).any() and not got["region"][miss].any()


def grown_boxes(nodes, seed, frac=0.5):
    """A caller's LOOSE tree whose boxes still contain their vertices: boxes of a valid tree grown at random, per face, by up to 30 % of their size (leaves
    too) — the boxes a point query is defined over (a box that leaves a vertex out culls a candidate the definition counts: not this form's contract)."""
    rng = np.random.RandomState(seed)
    out = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1).copy()
    pick = np.flatnonzero(rng.rand(out.shape[0]) < frac)
    b = out["bounds"][pick].astype(np.float64)
    size = b[:, 1::2] - b[:, 0::2]
    lo = (b[:, 0::2] - size * rng.uniform(0, 0.3, size.shape)).astype(np.float32)
    hi = (b[:, 1::2] + size * rng.uniform(0, 0.3, size.shape)).astype(np.float32)
    nb = out["bounds"][pick]
    nb[:, 0::2], nb[:, 1::2] = np.minimum(lo, nb[:, 0::2]), np.maximum(hi, nb[:, 1::2])  # (never inside the tight box, whatever the rounding did)
    out["bounds"][pick] = nb
    return out


def triangles_under(nodes):
    """for every node reachable from the root, the (stored) indices of the triangles under it"""
    rec = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)
    under = {}

    def walk(i):
        first, count = int(rec["first"][i]), int(rec["count"][i])
        under[i] = np.arange(first, first + count) if count > 0 else np.concatenate([walk(first), walk(first + 1)])
        return under[i]

    walk(0)
    return under
