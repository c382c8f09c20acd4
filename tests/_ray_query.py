"""The statement of a ray query (include/rvpt_hip.h: RAY QUERIES) and the rays the tests ask with.

The statement is the reference's walk written out in Python over the oracle's two tests — oracle.aabb_test and oracle.tri_test, both of which take the interval
(mint, maxt): that gives tmax and any hit, which oracle.closest_hit (always (0, inf), always the closest) does not have.  Traversal 0 is intersect_bvh
(intersection.glsl:361-413: a stack of right children, left child first), traversal 1 the loop over the triangles in stored order.  It goes through the same C
entry points those two wrappers call, with the pointers made once (a walk is tens of calls per ray and the wrappers convert their arrays on every call);
tests/test_ray_query_host.py checks it against the wrappers and against oracle.closest_hit."""
import ctypes as C

import numpy as np

from rvpt_amd import native

NO_PRIM = 0xFFFFFFFF


class Statement:
    """The scene a query is asked of: `nodes` (32-byte nodes, any layout the reference walks, or None) and `tris` (float32[n, 16]) in stored order."""

    def __init__(self, oracle, nodes, tris):
        self.L = oracle.lib()
        self.tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
        self.n_tris = self.tris.shape[0]
        self._tri0 = self.tris.ctypes.data
        self.n_nodes = 0
        if nodes is not None:
            rec = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)
            self.n_nodes = rec.shape[0]
            self.first, self.count = rec["first"].tolist(), rec["count"].tolist()
            self.bmin = np.ascontiguousarray(rec["bounds"][:, 0::2], dtype=np.float32)
            self.bmax = np.ascontiguousarray(rec["bounds"][:, 1::2], dtype=np.float32)
            self._bmin0, self._bmax0 = self.bmin.ctypes.data, self.bmax.ctypes.data
        self._o, self._d, self._tuv = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._po, self._pd, self._ptuv = self._o.ctypes.data, self._d.ctypes.data, self._tuv.ctypes.data

    def _tri(self, i, maxt):
        return self.L.oracle_tri_test(self._po, self._pd, self._tri0 + 64 * i, 0.0, maxt, self._ptuv)

    def _box(self, i, maxt):
        return self.L.oracle_aabb_test(self._po, self._pd, self._bmin0 + 12 * i, self._bmax0 + 12 * i, 0.0, maxt)

    def trace(self, org, dirv, tmax=np.inf, any_hit=False, traversal=0):
        """(prim, t, u, v): the closest hit in (0, tmax) — any_hit: the FIRST triangle the order accepts — or (NO_PRIM, tmax, 0, 0)."""
        tmax = np.float32(tmax)
        miss = (NO_PRIM, tmax, np.float32(0), np.float32(0))
        org, dirv = np.asarray(org, np.float32), np.asarray(dirv, np.float32)
        if not (np.isfinite(org).all() and np.isfinite(dirv).all() and tmax > 0):  # decided before the walk (a NaN tmax fails the comparison)
            return miss
        self._o[:], self._d[:] = org, dirv
        closest, best = float(tmax), None
        with np.errstate(all="ignore"):
            if traversal == 1:
                for i in range(self.n_tris):
                    if self._tri(i, closest):
                        closest, best = float(self._tuv[0]), (i, *self._tuv.copy())
                        if any_hit:
                            break
            elif self.n_nodes:
                stack, top = [], 0
                while True:
                    descend = False
                    if self._box(top, closest):
                        if self.count[top] > 0:
                            for i in range(self.first[top], self.first[top] + self.count[top]):
                                if self._tri(i, closest):
                                    closest, best = float(self._tuv[0]), (i, *self._tuv.copy())
                                    if any_hit:
                                        return best
                        else:
                            stack.append(self.first[top] + 1)
                            top, descend = self.first[top], True
                    if not descend:
                        if not stack:
                            break
                        top = stack.pop()
        return best if best is not None else miss

    def answer(self, records, traversal=0, perm=None):
        """`records` (RAY_HIT_DTYPE) with the out fields as a query leaves them; perm: prim goes through it (the caller's numbering after a build form)"""
        out = records.copy()
        for k in range(out.shape[0]):
            r = out[k]
            prim, t, u, v = self.trace(r["org"], r["dir"], r["tmax"], bool(r["flags"] & native.RAY_ANY_HIT), traversal)
            if prim == NO_PRIM:
                out["t"].view(np.uint32)[k] = records["tmax"].view(np.uint32)[k]  # the bits of tmax as given, a NaN's payload included
                out["prim"][k], out["u"][k], out["v"][k] = NO_PRIM, 0, 0
            else:
                out["t"][k], out["prim"][k], out["u"][k], out["v"][k] = t, (prim if perm is None else perm[prim]), u, v
        return out


def make_records(org, dirv, tmax=np.inf, flags=0):
    org = np.asarray(org, np.float32).reshape(-1, 3)
    rec = np.zeros(org.shape[0], dtype=native.RAY_HIT_DTYPE)
    rec["org"], rec["dir"], rec["tmax"], rec["flags"] = org, np.asarray(dirv, np.float32).reshape(-1, 3), tmax, flags
    return poisoned(rec)


def poisoned(records):
    """the out fields filled with a pattern no query leaves: a field the library did not write shows"""
    rec = records.copy()
    for name in ("t", "prim", "u", "v"):
        rec[name].view(np.uint32)[:] = 0xCDCDCDCD
    return rec


def same_bytes(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def first_difference(got, want):
    g, w = got.view(np.uint32).reshape(-1, 12), want.view(np.uint32).reshape(-1, 12)
    bad = np.flatnonzero((g != w).any(axis=1))
    return "no difference" if bad.size == 0 else f"{bad.size} of {g.shape[0]} records differ, the first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


def _vertices(tris):
    return np.asarray(tris, np.float32).reshape(-1, 4, 4)[:, :3, :3]


def shared_edge_midpoints(tris):
    """midpoints (float32) of the edges that two or more triangles share, vertex for vertex"""
    v = _vertices(tris)
    seen = {}
    for t in range(v.shape[0]):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            key = tuple(sorted((v[t, a].tobytes(), v[t, b].tobytes())))
            seen.setdefault(key, [0, v[t, a], v[t, b]])[0] += 1
    mids = [((e[1] + e[2]) * np.float32(0.5)) for e in seen.values() if e[0] >= 2]
    return np.asarray(mids, np.float32).reshape(-1, 3)


def base_rays(tris, seed, counts=(600, 600, 300, 200, 200, 185)):
    """Rays against `tris`: origins inside the scene's box with random directions; origins outside aimed into it; axis-aligned directions (one and two zero
    components); rays aimed exactly at mesh vertices and at the midpoints of shared edges (ties); rays aimed away from everything.  A third carry the any-hit
    bit.  Shuffled, so that a wave holds every kind.  The default counts add up to 2048 + 37."""
    rng = np.random.RandomState(seed)
    v = _vertices(tris).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    centre, ext = (lo + hi) / 2, float((hi - lo).max())
    n_in, n_out, n_axis, n_vert, n_edge, n_away = counts

    def sphere(n):
        d = rng.normal(size=(n, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    def outside(n):
        return centre + sphere(n) * ext * rng.uniform(1.2, 2.5, (n, 1))

    def inside(n):
        return lo + (hi - lo) * rng.uniform(0.02, 0.98, (n, 3))

    org, dirv = [inside(n_in)], [sphere(n_in) * rng.uniform(0.3, 3.0, (n_in, 1))]  # (dir need not be normalised)
    o = outside(n_out)
    org.append(o)
    dirv.append(inside(n_out) - o)
    o = np.where(rng.rand(n_axis, 1) < 0.5, inside(n_axis), outside(n_axis))
    d = sphere(n_axis)
    zero_one = rng.randint(0, 3, n_axis)
    d[np.arange(n_axis), zero_one] = 0.0
    two = rng.rand(n_axis) < 0.5  # ... and a second component: +-one axis
    d[two, (zero_one[two] + 1) % 3] = 0.0
    org.append(o)
    dirv.append(d)
    o = outside(n_vert)
    org.append(o)
    dirv.append(v[rng.randint(0, v.shape[0], n_vert)].astype(np.float64) - o.astype(np.float32))
    mids = shared_edge_midpoints(tris)
    if mids.shape[0] == 0:
        mids = v
    o = outside(n_edge)
    org.append(o)
    dirv.append(mids[rng.randint(0, mids.shape[0], n_edge)].astype(np.float64) - o.astype(np.float32))
    o = outside(n_away)
    org.append(o)
    dirv.append(o - centre)
    org, dirv = np.concatenate(org).astype(np.float32), np.concatenate(dirv).astype(np.float32)
    order = rng.permutation(org.shape[0])
    flags = np.where(np.arange(org.shape[0]) % 3 == 0, native.RAY_ANY_HIT, 0).astype(np.uint32)
    return make_records(org[order], dirv[order], np.inf, flags)


def with_tmax_variants(records, answered):
    """`records` followed, for every ray that hits (`answered`: the statement's answer), by that ray with tmax = t / 2, exactly t (the test is strict: not that
    triangle), nextafter(t, inf), 0, -1 and NaN"""
    hit = np.flatnonzero(answered["prim"] != NO_PRIM)
    t = answered["t"][hit]
    extra = []
    for tmax in (t / np.float32(2), t, np.nextafter(t, np.float32(np.inf)), np.zeros_like(t), -np.ones_like(t), np.full_like(t, np.nan)):
        r = records[hit].copy()
        r["tmax"] = tmax
        extra.append(r)
    return np.concatenate([records] + extra)


def non_finite_records(records, seed, n=12):
    """n of `records` with a NaN, +inf or -inf in one component of org or dir"""
    rng = np.random.RandomState(seed)
    out = records[rng.randint(0, records.shape[0], n)].copy()
    for k in range(n):
        out["org" if k % 2 else "dir"][k, rng.randint(0, 3)] = (np.nan, np.inf, -np.inf)[k % 3]
    return out
