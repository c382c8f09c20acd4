"""The statement of a k-nearest ray query (include/rvpt_hip.h: K-NEAREST RAY QUERIES), the records the tests ask with, and the layered scene.

The statement is _ray_query.Statement's walk — the same two oracle tests through the same pointers, the same two orders — with `closest` replaced by `bound`:
a ray keeps a list H of at most k accepted hits; in closest mode a hit goes behind every entry whose t is <= its own, the (k + 1)-th entry is dropped and
bound is the k-th t once H holds k; in any-hit mode bound stays tmax, hits are appended, and the walk stops at k."""
import numpy as np

import _ray_query as rq
from rvpt_amd import native

NO_PRIM = rq.NO_PRIM
POISON = 0xCDCDCDCD


class Statement(rq.Statement):
    def trace_k(self, org, dirv, k, tmax=np.inf, any_hit=False, traversal=0):
        """the list H: [(prim, t, u, v)] of at most k entries"""
        tmax = np.float32(tmax)
        org, dirv = np.asarray(org, np.float32), np.asarray(dirv, np.float32)
        if not (np.isfinite(org).all() and np.isfinite(dirv).all() and tmax > 0):  # decided before the walk
            return []
        self._o[:], self._d[:] = org, dirv
        H = []
        bound = [float(tmax)]

        def leaf(first, count):
            """True: an any-hit ray holds its k"""
            for i in range(first, first + count):
                if self._tri(i, bound[0]):
                    entry = (i, *self._tuv.copy())
                    if any_hit:
                        H.append(entry)
                        if len(H) == k:
                            return True
                    else:
                        at = len(H)
                        while at > 0 and H[at - 1][1] > entry[1]:  # behind every entry whose t is <= its own
                            at -= 1
                        H.insert(at, entry)
                        del H[k:]
                        if len(H) == k:
                            bound[0] = float(H[-1][1])
            return False

        with np.errstate(all="ignore"):
            if traversal == 1:
                leaf(0, self.n_tris)
            elif self.n_nodes:
                stack, top = [], 0
                while True:
                    descend = False
                    if self._box(top, bound[0]):
                        if self.count[top] > 0:
                            if leaf(self.first[top], self.count[top]):
                                return H
                        else:
                            stack.append(self.first[top] + 1)
                            top, descend = self.first[top], True
                    if not descend:
                        if not stack:
                            break
                        top = stack.pop()
        return H

    def answer_k(self, records, k, traversal=0, perm=None):
        """`records` (RAY_HIT_DTYPE, n * k of them, flat or [n, k]) as a k-nearest query leaves them: only the out quads change"""
        out = records.copy()
        g = out.reshape(-1, k)
        for r in g:
            H = self.trace_k(r[0]["org"], r[0]["dir"], k, r[0]["tmax"], bool(r[0]["flags"] & native.RAY_ANY_HIT), traversal)
            for j in range(k):
                if j < len(H):
                    prim, t, u, v = H[j]
                    r["t"][j], r["prim"][j], r["u"][j], r["v"][j] = t, (prim if perm is None else perm[prim]), u, v
                else:
                    r["t"].view(np.uint32)[j] = r["tmax"].view(np.uint32)[0]  # the bits of record 0's tmax as given, a NaN's payload included
                    r["prim"][j], r["u"][j], r["v"][j] = NO_PRIM, 0, 0
        return out


def groups(rays, k):
    """n * k records (flat) for the rays `rays` (RAY_HIT_DTYPE[n]): record 0 of a group is the ray; the followers' in fields and every out quad carry poison,
    so a field the library wrote, or failed to write, or read from a follower, shows"""
    out = np.empty((rays.shape[0], k), dtype=native.RAY_HIT_DTYPE)
    out.view(np.uint32)[...] = POISON
    out[:, 0] = rq.poisoned(rays)
    return out.reshape(-1)


def check_groups(got, want, records, what):
    got, want, records = got.reshape(-1), want.reshape(-1), records.reshape(-1)
    assert rq.same_bytes(got, want), f"{what}: {rq.first_difference(got, want)}"
    for name in ("org", "tmax", "dir", "flags"):  # the in fields come back byte for byte, the followers' poison included
        assert got[name].tobytes() == records[name].tobytes(), (what, name)


LAYERS = 12
DUPLICATED = (2, 5, 6, 9)  # layers that are an exact copy of the layer in front of them: equal t across list slots


def layered_scene(seed=4):
    """(tris, z of every triangle in stored order): 12 parallel quads (24 triangles) facing -z, stacked along z, in shuffled stored order — arrival order is not
    distance order.  Layer j of DUPLICATED sits exactly where layer j - 1 does."""
    from rvpt_amd import scene
    z = [1.0 + 0.5 * j for j in range(LAYERS)]
    for j in DUPLICATED:
        z[j] = z[j - 1]
    order = np.random.RandomState(seed).permutation(LAYERS)
    quads, zs = [], []
    for j in order:
        p = [(-1.0, -1.0, z[j]), (1.0, -1.0, z[j]), (1.0, 1.0, z[j]), (-1.0, 1.0, z[j])]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
        zs += [z[j], z[j]]
    return scene.make_triangles(quads, 0), np.asarray(zs, np.float64)


def through_rays(n, seed):
    """rays from z = 0 straight and slightly slanted through every layer, off the quads' diagonal (x != y): each meets exactly one triangle per layer"""
    rng = np.random.RandomState(seed)
    org = np.zeros((n, 3), np.float32)
    org[:, 0], org[:, 1] = rng.uniform(-0.4, -0.1, n), rng.uniform(0.1, 0.4, n)
    d = np.zeros((n, 3), np.float32)
    d[:, 0], d[:, 1], d[:, 2] = rng.uniform(-0.02, 0.0, n), rng.uniform(0.0, 0.02, n), 1.0
    return rq.make_records(org, d)
