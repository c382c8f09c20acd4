"""What the sphere-sweep tests share (include/rvpt_hip.h: SPHERE SWEEPS).  The statement itself is rvpt_amd/scene.py: sphere_sweeps — brute force over
sweep_sphere_triangles — and tests/test_sweep_host.py checks it; here are the record builder, the poison for the out quad, the generator of the GPU tests' record
sets with its census, a numpy walk with the strict skip, and float64 geometry that shares no formula with the statement."""
import numpy as np

from _ray_query import first_difference, same_bytes
from rvpt_amd import native, scene

NO_PRIM = 0xFFFFFFFF
IN_FIELDS = ("org", "radius", "dir", "tmax")
OUT_FIELDS = ("t", "prim", "u", "v")
INVALID_KINDS = ("org nan", "org inf", "dir nan", "dir inf", "radius nan", "radius negative", "radius inf", "tmax nan", "tmax negative")


def vertices(tris):
    return np.asarray(tris, np.float32).reshape(-1, 4, 4)[:, :3, :3]


def box_of(tris):
    """(centre float64[3], extent: the largest side of the scene's box)"""
    flat = vertices(tris).reshape(-1, 3).astype(np.float64)
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    return (lo + hi) / 2, float((hi - lo).max())


def poisoned(records):
    """the out quad filled with a pattern no query leaves: a field the library did not write shows"""
    rec = records.copy()
    for name in OUT_FIELDS:
        rec[name].view(np.uint32)[...] = 0xCDCDCDCD
    return rec


def make_records(org, direction, radius, tmax=np.inf):
    return poisoned(scene.sweep_records(org, direction, radius, tmax).astype(native.SPHERE_SWEEP_DTYPE))


def answer(tris, records, perm=None, features=None):
    """`records` with the out quad as a query leaves it: scene.sphere_sweeps on `tris` in stored order, prim numbered through `perm` where there is one"""
    with np.errstate(all="ignore"):
        want = scene.sphere_sweeps(tris, records, perm=perm, features=features)
    miss = want["prim"] == NO_PRIM
    want["t"].view(np.uint32)[miss] = records["tmax"].view(np.uint32)[miss]  # the bits as given, a NaN's payload included
    return want


def check(got, want, records, what):
    assert same_bytes(got, want), f"{what}: {first_difference(got, want)}"
    for name in IN_FIELDS:  # the in quads come back byte for byte, NaN payloads included
        assert got[name].tobytes() == records[name].tobytes(), (what, name)
    miss = got["prim"] == NO_PRIM  # a miss's out quad is all written: the bits of tmax, u = v = 0
    assert got["t"][miss].tobytes() == records["tmax"][miss].tobytes() and not got["u"][miss].view(np.uint32).any() and not got["v"][miss].view(np.uint32).any()


def surface_samples(tris, rng, n):
    """(points float64[n, 3] on random triangles, their unit normals, the triangle of each)"""
    v = vertices(tris).astype(np.float64)
    pick = rng.randint(0, v.shape[0], n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    pts = (v[pick] * w[:, :, None]).sum(axis=1)
    nrm = np.cross(v[pick, 1] - v[pick, 0], v[pick, 2] - v[pick, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    return pts, nrm, pick


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def aimed(tris, rng, n, r_lo=0.01, r_hi=1.0, reach=2.0):
    """n well-conditioned sweeps: origins within `reach` extents of the scene's centre (a box of four extents across at reach = 2), each aimed at a point of
    the mesh, dir of any length, radii log-uniform in [r_lo, r_hi] extents; (org, dir, radius) in float64"""
    centre, ext = box_of(tris)
    org = centre + ext * rng.uniform(-reach, reach, (n, 3))
    target = surface_samples(tris, rng, n)[0] + 0.05 * ext * rng.normal(size=(n, 3))
    d = (target - org) * rng.uniform(0.25, 2.0, (n, 1))
    radius = ext * 10.0 ** rng.uniform(np.log10(r_lo), np.log10(r_hi), n)
    return org, d, radius


def sweeps_of(tris, seed, n_aimed=500, n_feature=240, n_overlap=90, n_still=60, n_away=70, n_short=60, n_exact=40, n_invalid=3):
    """The GPU tests' records against `tris`, shuffled so that a wave holds every kind:
    aimed — within four extents, aimed at the mesh, every radius from a hundredth to one extent, tmax +inf or around the contact;
    feature — thin spheres (a thousandth to a fiftieth of an extent) sent from outside straight at vertices, at edge midpoints and at face centres;
    overlap — spheres that stand in the surface and move on (t = 0, and ties between the triangles they stand in);
    still — dir = 0, 0, 0, inside the surface and outside it;
    away — aimed records turned round; short — aimed records with a tmax that ends before the contact; exact — tmax at the reported time, bit for bit, and one
    ulp below it; -0.0 for radius and for tmax;
    invalid — n_invalid of every kind of INVALID_KINDS."""
    rng = np.random.RandomState(seed)
    centre, ext = box_of(tris)
    v = vertices(tris).astype(np.float64)
    org, d, radius = aimed(tris, rng, n_aimed)
    tmax = np.where(rng.rand(n_aimed) < 0.5, np.inf, rng.uniform(0.0, 2.5, n_aimed))
    parts = [(org, d, radius, tmax)]
    # feature: from 1 .. 3 extents out along a direction that leaves the scene, at a vertex, an edge midpoint or a centroid
    pick, which = rng.randint(0, v.shape[0], n_feature), rng.randint(0, 3, n_feature)
    corner = v[pick, which]
    goal = np.where((np.arange(n_feature) % 3 == 0)[:, None], corner,
                    np.where((np.arange(n_feature) % 3 == 1)[:, None], (corner + v[pick, (which + 1) % 3]) / 2, v[pick].mean(axis=1)))
    out = goal - centre + 0.3 * ext * rng.normal(size=(n_feature, 3))
    out /= np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-300)
    f_org = goal + out * ext * rng.uniform(1.0, 3.0, (n_feature, 1))
    parts.append((f_org, (goal - f_org) * rng.uniform(0.5, 1.5, (n_feature, 1)), ext * 10.0 ** rng.uniform(-3, -1.7, n_feature), np.full(n_feature, np.inf)))
    # overlap: the centre within the radius of a surface point
    pts, nrm, _ = surface_samples(tris, rng, n_overlap)
    o_r = ext * 10.0 ** rng.uniform(-2, -0.5, n_overlap)
    parts.append((pts + nrm * (o_r * rng.uniform(-0.9, 0.9, n_overlap))[:, None], ext * _unit(rng, n_overlap), o_r, np.full(n_overlap, np.inf)))
    # still: dir = 0, inside and outside
    pts, nrm, _ = surface_samples(tris, rng, n_still)
    s_r = ext * 10.0 ** rng.uniform(-2, -1, n_still)
    off = np.where(np.arange(n_still) % 2 == 0, rng.uniform(0.0, 0.9, n_still), rng.uniform(1.5, 40.0, n_still))
    parts.append((pts + nrm * (s_r * off)[:, None], np.zeros((n_still, 3)), s_r, np.where(np.arange(n_still) % 3 == 0, 0.0, np.inf)))
    a_org, a_d, a_r = aimed(tris, rng, n_away)
    parts.append((a_org, -a_d, a_r * 0.1, np.full(n_away, np.inf)))
    org64, d64, r64, t64 = (np.concatenate([p[k] for p in parts]) for k in range(4))
    base = make_records(org64, d64, r64, t64)
    got = answer(tris, base)
    hit = np.flatnonzero((got["prim"] != NO_PRIM) & (got["t"] > 0))
    extra = []
    for count, bound in ((n_short, lambda t: t * np.float32(0.5)), (n_exact // 2, lambda t: t), (n_exact - n_exact // 2, lambda t: np.nextafter(t, np.float32(0)))):
        rows = hit[rng.randint(0, hit.shape[0], count)] if hit.size else hit
        r = base[rows].copy()
        r["tmax"] = bound(got["t"][rows])
        extra.append(r)
    zeros = base[rng.randint(0, base.shape[0], 8)].copy()
    zeros["radius"][:4], zeros["tmax"][4:] = np.float32(-0.0), np.float32(-0.0)
    extra.append(zeros)
    bad = base[rng.randint(0, base.shape[0], n_invalid * len(INVALID_KINDS))].copy()
    for k in range(bad.shape[0]):
        kind, axis = INVALID_KINDS[k % len(INVALID_KINDS)], rng.randint(0, 3)
        if kind == "org nan":
            bad["org"][k, axis] = np.nan
        elif kind == "org inf":
            bad["org"][k, axis] = (np.inf, -np.inf)[k % 2]
        elif kind == "dir nan":
            bad["dir"][k, axis] = np.nan
        elif kind == "dir inf":
            bad["dir"][k, axis] = (np.inf, -np.inf)[k % 2]
        elif kind == "radius nan":
            bad["radius"][k] = np.nan
        elif kind == "radius negative":
            bad["radius"][k] = -abs(bad["radius"][k]) - np.float32(1e-3)
        elif kind == "radius inf":
            bad["radius"][k] = np.inf
        elif kind == "tmax nan":
            bad["tmax"].view(np.uint32)[k] = 0x7FC12345  # a payload that must come back
        else:
            bad["tmax"][k] = -1.5
    extra.append(bad)
    records = poisoned(np.concatenate([base] + extra))
    return records[rng.permutation(records.shape[0])]


def invalid_kind(records):
    """per record the index into INVALID_KINDS of the first rule it breaks, -1 for a valid one"""
    with np.errstate(all="ignore"):
        rules = [np.isnan(records["org"]).any(axis=1), np.isinf(records["org"]).any(axis=1), np.isnan(records["dir"]).any(axis=1), np.isinf(records["dir"]).any(axis=1),
                 np.isnan(records["radius"]), records["radius"] < 0, np.isinf(records["radius"]), np.isnan(records["tmax"]), records["tmax"] < 0]
    kind = np.full(records.shape[0], -1)
    for k in reversed(range(len(rules))):
        kind[rules[k]] = k
    return kind


def sweep_set(tris, seed, **counts):
    """(records, want, features): sweeps_of, the statement's answer, and the deciding feature of every hit; read-only"""
    records = sweeps_of(tris, seed, **counts)
    features = np.zeros(records.shape[0], dtype=np.int64)
    want = answer(tris, records, features=features)
    for a in (records, want, features):
        a.setflags(write=False)
    return records, want, features


def ties(tris, records, want, limit=400):
    """how many of the first `limit` hits have a second triangle whose candidate has the winner's t, bit for bit"""
    hit = np.flatnonzero(want["prim"] != NO_PRIM)[:limit]
    with np.errstate(all="ignore"):
        has, t, _, _, _ = scene.sweep_sphere_triangles(records["org"][hit], records["dir"][hit], records["radius"][hit], records["tmax"][hit], tris)
    return int(((has & (t == want["t"][hit, None])).sum(axis=1) > 1).sum())


def census(records, want, features):
    """{"n", "hits", "misses", "overlaps" (t == 0 hits), "invalid": per kind, "features": hits per deciding feature}; misses count valid records only"""
    kind = invalid_kind(records)
    hit = want["prim"] != NO_PRIM
    return {"n": records.shape[0], "hits": int(hit.sum()), "misses": int((~hit & (kind < 0)).sum()), "overlaps": int((hit & (want["t"] == 0)).sum()),
            "invalid": [int((kind == k).sum()) for k in range(len(INVALID_KINDS))], "features": np.bincount(features[hit], minlength=7).tolist()}


def holds_conditions(c):
    """the issue's conditions on a GPU record set: every feature decides, >= 5 % misses, >= 5 % initial overlaps, invalid records of every kind"""
    return min(c["features"]) >= 1 and c["misses"] >= 0.05 * c["n"] and c["overlaps"] >= 0.05 * c["n"] and min(c["invalid"]) >= 1


# ---- a numpy walk with the strict skip ------------------------------------------------------------------------------------------------------------------------

def walk(nodes, tris, record, perm=None, order="near"):
    """One record against a tree (NODE_DTYPE, root 0, children at first, first + 1) over `tris` in stored order, as the kernel walks: a node is skipped iff its
    slab test fails or t_in(node) > best — strictly — and a leaf's triangles give sweep_sphere_triangles' candidates.  order: "near" (the smaller t_in first),
    "far", "left" or "right": the answer does not depend on it.  Returns (t, prim, u, v) with prim = NO_PRIM for a miss, and the number of leaves visited."""
    rec = np.ascontiguousarray(nodes).view(native.NODE_DTYPE).reshape(-1)
    p, d, r, big_t = record["org"], record["dir"], record["radius"], record["tmax"]
    best, best_prim, best_uv, leaves = np.float32(big_t), NO_PRIM, (np.float32(0), np.float32(0)), 0

    def slab(i):
        b = rec["bounds"][i]
        ok, t_in = scene.sweep_slab(p, d, r, big_t, b[0::2], b[1::2])
        return bool(ok), np.float32(t_in)

    ok, t_root = slab(0)
    stack = [(t_root, 0)] if ok else []
    while stack:
        t_node, i = stack.pop()
        if t_node > best:
            continue
        first, count = int(rec["first"][i]), int(rec["count"][i])
        if count > 0:
            leaves += 1
            with np.errstate(all="ignore"):
                has, t, u, v, _ = scene.sweep_sphere_triangles(p, d, r, big_t, tris[first:first + count])
            for j in np.flatnonzero(has):
                number = first + j if perm is None else int(perm[first + j])
                if t[j] < best or (t[j] == best and number < best_prim):
                    best, best_prim, best_uv = t[j], number, (u[j], v[j])
            continue
        kids = []
        for c in (first, first + 1):
            ok, t_c = slab(c)
            if ok and not t_c > best:
                kids.append((t_c, c))
        if len(kids) == 2:
            swap = {"near": kids[0][0] > kids[1][0], "far": kids[0][0] <= kids[1][0], "left": False, "right": True}[order]
            if swap:
                kids.reverse()
        stack.extend(reversed(kids))  # the first of `kids` is popped first
    return best, best_prim, best_uv[0], best_uv[1], leaves


# ---- float64 geometry that shares no formula with the statement ----------------------------------------------------------------------------------------------

def distances(points, verts):
    """The distance from points float64[m, 3] to triangles verts[n, 3, 3], float64[m, n]: the distance to the plane where the foot lies inside the three edge
    half-planes, else the smallest distance to the three segments by clamped projection"""
    p = np.asarray(points, np.float64)[:, None, :]
    v = np.asarray(verts, np.float64)
    a, b, c = v[:, 0], v[:, 1], v[:, 2]

    def segment(x0, x1):
        e, w = x1 - x0, p - x0
        ee = (e * e).sum(-1)
        s = np.clip((w * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        return np.linalg.norm(w - e * s[..., None], axis=-1)

    edge = np.minimum(np.minimum(segment(a, b), segment(b, c)), segment(c, a))
    n = np.cross(b - a, c - a)
    length = np.linalg.norm(n, axis=-1)
    unit = n / np.where(length > 0, length, 1.0)[:, None]
    h = ((p - a) * unit).sum(-1)
    foot = p - h[..., None] * unit

    def side(x0, x1):
        return (np.cross(x1 - x0, foot - x0) * unit).sum(-1)

    inside = (side(a, b) >= 0) & (side(b, c) >= 0) & (side(c, a) >= 0) & (length > 0)
    return np.where(inside, np.minimum(np.abs(h), edge), edge)


def horizon(tris, org, d, radius, tmax):
    """a finite end of every sweep for sampling: tmax, or the time after which the sphere has left the scene for good"""
    centre, ext = box_of(tris)
    speed = np.maximum(np.linalg.norm(d, axis=1), 1e-300)
    leave = (np.linalg.norm(org - centre, axis=1) + 2.0 * ext + radius) / speed
    return np.where(np.isfinite(tmax), tmax, leave)


def closest_approach(tris, org, d, end, samples=256, rounds=32):
    """float64[m]: the smallest distance between the centre's path over [0, end] and the mesh — `samples` evenly spaced times, then a ternary search about the
    best of them (the distance to one triangle is convex along a line; about its smallest sample the distance to the mesh is taken to be)"""
    v = vertices(tris)
    org, d = np.asarray(org, np.float64), np.asarray(d, np.float64)
    m = org.shape[0]
    best, at = np.full(m, np.inf), np.zeros(m)
    for k in range(samples + 1):
        t = end * k / samples
        dist = distances(org + d * t[:, None], v).min(axis=1)
        better = dist < best
        best, at = np.where(better, dist, best), np.where(better, t, at)
    lo, hi = np.maximum(at - end / samples, 0.0), np.minimum(at + end / samples, end)
    for _ in range(rounds):
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        f1, f2 = distances(org + d * m1[:, None], v).min(axis=1), distances(org + d * m2[:, None], v).min(axis=1)
        lo, hi = np.where(f1 <= f2, lo, m1), np.where(f1 <= f2, m2, hi)
        best = np.minimum(best, np.minimum(f1, f2))
    return best


def geometric_errors(tris, records, want):
    """The statement's answers against float64 geometry, in units of each record's radius.  Returns (err float64[m], approach float64[m]): err is the largest of
    (a) | distance(centre at t, triangle prim) - r | for a hit with t > 0, and the excess of that distance over r for a hit at t = 0,
    (b) the depth r - distance below r, over every triangle, at 64 evenly spaced times before t,
    (c) for a miss, that depth at 256 times over [0, tmax] (a finite horizon where tmax is +inf);
    approach is (closest approach - r) / r over the whole sweep: a record with |approach| within a tolerance is a marginal graze."""
    v = vertices(tris)
    org, d = records["org"].astype(np.float64), records["dir"].astype(np.float64)
    r, t = records["radius"].astype(np.float64), want["t"].astype(np.float64)
    end = horizon(tris, org, d, r, records["tmax"].astype(np.float64))
    hit = want["prim"] != NO_PRIM
    err = np.zeros(org.shape[0])
    rows = np.flatnonzero(hit)
    at = distances(org[rows] + d[rows] * t[rows, None], v)[np.arange(rows.size), want["prim"][rows]]
    err[rows] = np.where(t[rows] > 0, np.abs(at - r[rows]), np.maximum(at - r[rows], 0.0))
    for k in range(64):
        tk = t[rows] * k / 64
        depth = r[rows] - distances(org[rows] + d[rows] * tk[:, None], v).min(axis=1)
        err[rows] = np.maximum(err[rows], np.where(t[rows] > 0, depth, 0.0))
    rows = np.flatnonzero(~hit)
    for k in range(257):
        tk = end[rows] * k / 256
        depth = r[rows] - distances(org[rows] + d[rows] * tk[:, None], v).min(axis=1)
        err[rows] = np.maximum(err[rows], depth)
    approach = (closest_approach(tris, org, d, end) - r) / r
    return err / r, approach


# ---- the scenes and record sets of the GPU tests, made once ----------------------------------------------------------------------------------------------------

def chain_triangles():
    """the box queries' 24 quads along z, of growing size: 48 triangles for a chain of 48 leaves"""
    rng = np.random.RandomState(11)
    quads = []
    for i in range(24):
        z, s, c = 1.0 + 0.25 * i, 0.3 + 0.05 * i, rng.uniform(-0.5, 0.5, 2)
        p = [(c[0] - s, c[1] - s, z), (c[0] + s, c[1] - s, z), (c[0] + s, c[1] + s, z), (c[0] - s, c[1] + s, z)]
        quads += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    return scene.make_triangles(quads, 0)


SET_NAMES = ("default", "caller", "layers", "chain", "field512", "field578")
_SETS = {}


def triangles_named(name):
    """default: the default scene in the leaf order of the host builder (143); caller: the same in the caller's order; layers: the multi-hit tests' 12 layers
    with four exact duplicates; chain: chain_triangles; field512 / field578: height fields of exactly one brute-force tile and of one tile and a tail"""
    if name == "default":
        tris = scene.default_scene()[0]
        return np.ascontiguousarray(tris[native.build_bvh(tris)[1]])
    if name == "caller":
        return scene.default_scene()[0]
    if name == "layers":
        import _multi_hit as mh
        return mh.layered_scene()[0]
    if name == "chain":
        return chain_triangles()
    return scene.heightfield_scene(cells={"field512": 16, "field578": 17}[name])[0]


def set_named(name):
    """(tris, records, want, features) of a GPU test's scene: sweeps_of with a seed of its own and smaller counts on the larger scenes; computed once"""
    if name not in _SETS:
        tris = triangles_named(name)
        small = dict(n_aimed=150, n_feature=90, n_overlap=40, n_still=20, n_away=20, n_short=20, n_exact=10, n_invalid=1)
        counts = {} if name in ("default", "caller") else small
        _SETS[name] = (tris,) + sweep_set(tris, 7 + 2 * SET_NAMES.index(name), **counts)
    return _SETS[name]
