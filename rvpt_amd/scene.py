"""Host-side scene construction: the POD arrays RVPT uploads to the GPU.

Mirrors the reference's host structs and scene set-up (paths relative to the reference tree):
  * Triangle  — src/rvpt/geometry.h:76-111 (4 x vec4; the face normal rides in the .w lanes)
  * Material  — src/rvpt/material.h:9-26
  * load_model / default scene — src/rvpt/main.cpp:12-62, 102-107
plus the deterministic synthetic scenes BASELINE.json's configs name (Cornell box + subdivided model,
~1M-triangle heightfield).  Pure numpy; no GPU.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

LAMBERT, MIRROR, DIELECTRIC = 0, 1, 2  # Material::Type, material.h:11-16

_ASSETS = Path(__file__).resolve().parent / "assets"


def make_triangles(positions, material_id: int) -> np.ndarray:
    """positions[n,3,3] -> float32[n,16] in the reference Triangle layout (geometry.h:81-91)."""
    p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3, 3)
    n = p.shape[0]
    out = np.zeros((n, 16), dtype=np.float32)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(np.float32)
    ln = np.sqrt((nrm * nrm).sum(axis=1, keepdims=True)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = (nrm / ln).astype(np.float32)
    out[:, 0:3], out[:, 4:7], out[:, 8:11] = p[:, 0], p[:, 1], p[:, 2]
    out[:, 3], out[:, 7], out[:, 11] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    out[:, 12] = float(material_id)
    return out


def make_material(albedo, emission, mtype: int) -> np.ndarray:
    """float32[12] = albedo(4), emission(4), data(4) with data.x = type (material.h:17-25).
    albedo[3] doubles as the index of refraction (intersection.glsl:54)."""
    m = np.zeros(12, dtype=np.float32)
    m[0:4] = albedo
    m[4:8] = emission
    m[8] = float(mtype)
    return m


NODE_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("bounds", "<f4", (6,))])  # rvpt_bvh_node (== native.NODE_DTYPE)


def _min_no_nan(a, b):
    """np.minimum where neither is a NaN (the same bytes), otherwise the one that is not: fminf"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.minimum(a, b)))


def _max_no_nan(a, b):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.maximum(a, b)))


def _reduce_no_nan(x, axis):
    """(min, max) of x along axis: ndarray.min / max where no NaN took part (the same bytes), np.fmin / np.fmax — a NaN takes no part — elsewhere"""
    with np.errstate(invalid="ignore"):
        lo, hi = x.min(axis=axis), x.max(axis=axis)
        bad = np.isnan(lo)  # (min and max meet a NaN in the same places)
        if bad.any():
            lo, hi = np.where(bad, np.fmin.reduce(x, axis=axis), lo), np.where(bad, np.fmax.reduce(x, axis=axis), hi)
    return lo, hi


def refit_bvh(nodes, tris, touched=None) -> np.ndarray:
    """The normative refit of a tree whose triangles moved (the host statement of what rvpt_hip_upload_scene's update form does on the device): topology
    (`first`, `count`) kept, a leaf's box = component-wise min / max over the vertices of its triangles, an inner node's box = min / max of its two
    children's boxes.  min / max of floats is exact, so the result does not depend on the order of evaluation (up to the sign of a zero) and a tree whose
    boxes were tight comes back byte for byte; loose boxes become tight.  A NaN takes no part (the device's fminf / fmaxf, the rule of
    rvpt_amd/csrc/rvpt_build.h): a bound is NaN only where nothing but NaN took part — every coordinate of a leaf on that axis, or both children's bounds.
    Infinities are ordinary values.

    nodes: uint32[n, 8] (native.build_bvh) or NODE_DTYPE records, root at 0, children of an inner node at first, first + 1, leaf iff count > 0;
    tris: float32[m, 16] in the leaf order the tree indexes.  Returns a new array in the form of `nodes`; nodes the root does not reach are left as they are.
    Iterative (level by level), a few seconds for the 1.5 M nodes of the 1 M-triangle terrain.

    touched: None, or positions in leaf order (integers, any order, repeats allowed) — the host statement of the SPARSE update (include/rvpt_hip.h): only the
    leaves that hold a touched triangle and the nodes between such a leaf and the root are recomputed, by the same rule and deepest first; every other box comes
    back as it was given, loose ones included.  On a tree whose boxes were tight the result is the full refit's."""
    src = np.ascontiguousarray(nodes)
    out = src.copy()
    rec = out.view(NODE_DTYPE).reshape(-1)
    n = rec.shape[0]
    v = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3]
    first, count = rec["first"].astype(np.int64), rec["count"].astype(np.int64)
    if n == 0:
        return out
    # the levels of the tree, root first
    levels, frontier, seen = [], np.zeros(1, dtype=np.int64), 1
    while frontier.size:
        levels.append(frontier)
        inner = frontier[count[frontier] == 0]
        if inner.size and int(first[inner].max()) + 1 >= n:
            raise ValueError("refit_bvh: child index outside the node array")
        frontier = np.stack([first[inner], first[inner] + 1], axis=1).reshape(-1)
        seen += frontier.size
        if seen > n:
            raise ValueError("refit_bvh: not a tree (a node is reachable twice)")
    if touched is not None:
        return _refit_touched(out, rec, v, first, count, levels, touched)
    lo = np.empty((n, 3), dtype=np.float32)
    hi = np.empty((n, 3), dtype=np.float32)
    leaves = np.concatenate([l[count[l] > 0] for l in levels])
    if leaves.size:
        if int((first[leaves] + count[leaves]).max()) > v.shape[0]:
            raise ValueError("refit_bvh: leaf range outside the triangle array")
        tlo, thi = _reduce_no_nan(v, 1)
        lo[leaves], hi[leaves] = tlo[first[leaves]], thi[first[leaves]]
        for k in range(1, int(count[leaves].max())):  # the k-th triangle of every leaf that has one
            more = leaves[count[leaves] > k]
            lo[more] = _min_no_nan(lo[more], tlo[first[more] + k])
            hi[more] = _max_no_nan(hi[more], thi[first[more] + k])
    for level in reversed(levels):
        inner = level[count[level] == 0]
        lo[inner] = _min_no_nan(lo[first[inner]], lo[first[inner] + 1])
        hi[inner] = _max_no_nan(hi[first[inner]], hi[first[inner] + 1])
    reached = np.concatenate(levels)
    b = rec["bounds"]
    b[reached, 0::2], b[reached, 1::2] = lo[reached], hi[reached]
    return out


def _refit_touched(out, rec, v, first, count, levels, touched):
    """refit_bvh's sparse form: `levels` are the node indices per level, root first"""
    n = rec.shape[0]
    pos = np.unique(np.asarray(touched, dtype=np.int64).reshape(-1))
    if pos.size == 0:
        return out
    if int(pos[0]) < 0 or int(pos[-1]) >= v.shape[0]:
        raise ValueError("refit_bvh: touched position outside the triangle array")
    reached = np.concatenate(levels)
    leaves = reached[count[reached] > 0]
    if leaves.size and int((first[leaves] + count[leaves]).max()) > v.shape[0]:
        raise ValueError("refit_bvh: leaf range outside the triangle array")
    parent = np.full(n, -1, dtype=np.int64)
    inner = reached[count[reached] == 0]
    parent[first[inner]], parent[first[inner] + 1] = inner, inner
    # the leaf of every touched position: the leaves' ranges are disjoint, so sorted by `first` the last range that starts at or before a position holds it
    order = np.argsort(first[leaves], kind="stable")
    starts, sorted_leaves = first[leaves][order], leaves[order]
    slot = np.searchsorted(starts, pos, side="right") - 1
    held = slot >= 0
    cand = sorted_leaves[slot[held]]
    cand = cand[pos[held] < first[cand] + count[cand]]
    dirty = np.zeros(n, dtype=bool)
    front = np.unique(cand)
    while front.size:
        dirty[front] = True
        up = parent[front]
        up = np.unique(up[up >= 0])
        front = up[~dirty[up]]
    b = rec["bounds"]
    tlo, thi = _reduce_no_nan(v, 1)
    for level in reversed(levels):
        lv = level[dirty[level]]
        for i in lv[count[lv] > 0]:
            f, c = int(first[i]), int(count[i])
            b[i, 0::2], b[i, 1::2] = _reduce_no_nan(tlo[f:f + c], 0)[0], _reduce_no_nan(thi[f:f + c], 0)[1]
        inn = lv[count[lv] == 0]
        if inn.size:
            l, r = first[inn], first[inn] + 1
            b[inn, 0::2] = _min_no_nan(b[l, 0::2], b[r, 0::2])
            b[inn, 1::2] = _max_no_nan(b[l, 1::2], b[r, 1::2])
    return out


def tree_cost(nodes) -> float:
    """The SAH cost of a tree, the number the guarded update of rvpt_hip_upload_scene reports (include/rvpt_hip.h has the definition): every node the root reaches
    is one term; a node's extents are hi - lo per axis, taken in double from the float32 bounds, its half-area ex*ey + ey*ez + ez*ex in double; an inner node
    contributes its half-area, a leaf its half-area times its triangle count; the sum, in double, is divided by the root's half-area.  A root of half-area 0
    costs 0.  The device adds in another order: the two agree to n * 2^-53 relative, not to the bit.

    nodes: uint32[n, 8] (native.build_bvh) or NODE_DTYPE records, root at 0.  The levels are walked as refit_bvh walks them, so nodes the root does not reach
    are left out."""
    rec = np.ascontiguousarray(nodes).view(NODE_DTYPE).reshape(-1)
    n = rec.shape[0]
    if n == 0:
        return 0.0
    first, count = rec["first"].astype(np.int64), rec["count"].astype(np.int64)
    levels, frontier, seen = [], np.zeros(1, dtype=np.int64), 1
    while frontier.size:
        levels.append(frontier)
        inner = frontier[count[frontier] == 0]
        if inner.size and int(first[inner].max()) + 1 >= n:
            raise ValueError("tree_cost: child index outside the node array")
        frontier = np.stack([first[inner], first[inner] + 1], axis=1).reshape(-1)
        seen += frontier.size
        if seen > n:
            raise ValueError("tree_cost: not a tree (a node is reachable twice)")
    reached = np.concatenate(levels)
    b = rec["bounds"][reached].astype(np.float64)
    e = b[:, 1::2] - b[:, 0::2]
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    root = float(area[0])
    if not root > 0.0:
        return 0.0
    c = count[reached]
    return float(np.sum(area * np.where(c > 0, c, 1).astype(np.float64)) / root)


LBVH_LEAF_TRIS = 2  # == rv::kLbvhLeafTris (rvpt_amd/csrc/rvpt_build.h)


def lbvh_keys(tris) -> np.ndarray:
    """The 64-bit sort keys of the device BVH build (rvpt_amd/csrc/rvpt_build.h has the definition): per triangle i of the CALLER'S order, the 30-bit Morton code
    of its centroid quantised to 10 bits per axis over the centroid bounds (x the highest bit of each triple), shifted above the index i.  uint64[n]."""
    v = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3]
    n = v.shape[0]
    third = np.float32(1.0) / np.float32(3.0)
    with np.errstate(all="ignore"):
        c = ((v[:, 0] + v[:, 1]) + v[:, 2]) * third  # float32, left to right
        code = np.zeros(n, dtype=np.uint64)
        for ax in range(3):
            ca = c[:, ax]
            lo, hi = (np.fmin.reduce(ca), np.fmax.reduce(ca)) if n else (np.float32(0), np.float32(0))  # NaN centroids take no part
            ext = np.float32(hi - lo)
            q = np.zeros(n, dtype=np.uint64)
            if ext > 0:
                f = (ca - lo) * (np.float32(1024.0) / ext)
                inside = (f >= 0) & (f < 1023)  # false for a NaN
                q[inside] = f[inside].astype(np.int32).astype(np.uint64)
                q[f >= 1023] = 1023
            s = np.zeros(n, dtype=np.uint64)
            for bit in range(10):  # bit b of q -> bit 3 b (+ 2 for x, + 1 for y) of the code
                s |= ((q >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + (2 - ax))
            code |= s
    return (code << np.uint64(32)) | np.arange(n, dtype=np.uint64)


def _top_bit(x) -> np.ndarray:
    """index of the highest set bit of every element of uint64 x (all non-zero)"""
    hi = (x >> np.uint64(32)).astype(np.uint32)
    lo = (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    word = np.where(hi > 0, hi, lo).astype(np.float64)  # exact: 32 bits fit a double, and floor(log2) of one is exact
    return (np.floor(np.log2(word)).astype(np.int64) + np.where(hi > 0, 32, 0)).astype(np.uint64)


def build_lbvh(tris, leaf_tris: int = LBVH_LEAF_TRIS):
    """The tree rvpt_hip_upload_scene's BUILD FORM makes on the device, in numpy (the second statement of the one specification in
    rvpt_amd/csrc/rvpt_build.h): sort the keys (lbvh_keys; unique, so the order is unique), a node is a range [a, b] of the sorted keys, a leaf iff it holds
    <= leaf_tris of them, else split in front of the first key whose bit p is set, p = the highest bit in which key[a] and key[b] differ.  Boxes: refit_bvh.

    tris: float32[n, 16] in the CALLER'S order, n >= 1.  Returns (nodes NODE_DTYPE[m] in the reference layout: root 0, children of an inner node adjacent at
    first, first + 1, leaf iff count > 0, breadth first; perm uint32[n]: leaf-order triangle j is the caller's triangle perm[j]), so that
    upload_scene(nodes, tris[perm], mats) is the scene the build form uploads.  Vectorised per level; a few seconds for 1 M triangles."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    n = t.shape[0]
    if n == 0:
        raise ValueError("build_lbvh: no triangles")
    keys = np.sort(lbvh_keys(t))
    perm = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    firsts, counts = [], []
    a, b = np.zeros(1, dtype=np.int64), np.full(1, n - 1, dtype=np.int64)
    next_index, height = 1, 0
    while a.size:
        height += 1
        if height > 64:
            raise ValueError("build_lbvh: the tree is higher than 64 levels")
        inner = (b - a + 1) > leaf_tris
        ia, ib = a[inner], b[inner]
        p = _top_bit(keys[ia] ^ keys[ib])
        lo, hi = ia.copy(), ib.copy()  # bit p of key[lo] is 0, of key[hi] 1
        while True:
            open_ = (hi - lo) > 1
            if not open_.any():
                break
            mid = lo + (hi - lo) // 2
            bit = ((keys[mid] >> p) & np.uint64(1)).astype(bool)
            hi = np.where(open_ & bit, mid, hi)
            lo = np.where(open_ & ~bit, mid, lo)
        first = a.copy()
        first[inner] = next_index + 2 * np.arange(ia.size, dtype=np.int64)
        firsts.append(first)
        counts.append(np.where(inner, 0, b - a + 1))
        next_index += 2 * ia.size
        a = np.stack([ia, hi], axis=1).reshape(-1)
        b = np.stack([hi - 1, ib], axis=1).reshape(-1)
    nodes = np.zeros(next_index, dtype=NODE_DTYPE)
    nodes["first"], nodes["count"] = np.concatenate(firsts), np.concatenate(counts)
    return refit_bvh(nodes, t[perm]), perm


PLOC_RADIUS = 16           # == rv::kPlocRadius (rvpt_amd/csrc/rvpt_build.h)
PLOC_MAX_ITERATIONS = 256  # == rv::kPlocMaxIterations
PLOC_MAX_HEIGHT = 62       # == rv::kPlocMaxHeight: the depth check_bvh allows, inside the 64 levels the traversal stack walks


def _ploc_nearest(lo, hi, radius):
    """nn[i] = the j != i, |i - j| <= radius, with the smallest triple (d(i, j), i xor j, min(i, j)); d = half-area of the union box in double, +inf if not finite"""
    m = lo.shape[0]
    best_d = np.full(m, np.inf)
    best_x = np.full(m, np.iinfo(np.int64).max, dtype=np.int64)
    best_m = np.full(m, np.iinfo(np.int64).max, dtype=np.int64)
    nn = np.full(m, -1, dtype=np.int64)
    idx = np.arange(m, dtype=np.int64)
    with np.errstate(all="ignore"):
        for s in range(1, min(radius, m - 1) + 1):
            e = np.fmax(hi[:-s], hi[s:]).astype(np.float64) - np.fmin(lo[:-s], lo[s:]).astype(np.float64)
            d = (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]
            d = np.where(np.isfinite(d), d, np.inf)
            i, j = idx[:-s], idx[s:]
            x = i ^ j
            for me, other in ((i, j), (j, i)):  # the pair (i, i + s) is a candidate of both members; min(i, j) = i
                better = (d < best_d[me]) | ((d == best_d[me]) & ((x < best_x[me]) | ((x == best_x[me]) & (i < best_m[me]))))
                w = me[better]
                best_d[w], best_x[w], best_m[w], nn[w] = d[better], x[better], i[better], other[better]
    return nn


def build_ploc(tris, radius: int = PLOC_RADIUS, info: dict | None = None):
    """The tree rvpt_hip_upload_scene's PLOC BUILD FORM (RVPT_HIP_NODES_BUILD_PLOC) makes on the device, in numpy — the second statement of the specification in
    rvpt_amd/csrc/rvpt_build.h: parallel locally-ordered clustering (Meister & Bittner 2018) over build_lbvh's leaf order.  One cluster per sorted triangle;
    per iteration every cluster picks its nearest neighbour within `radius` positions by the triple (half-area of the union box in double, i xor j, min(i, j)),
    every mutual pair i < j becomes an inner node at position i (left i, right j), the array is compacted in order; until one cluster is left.  The tree is then
    laid out level by level in the reference layout, leaves of one triangle; boxes: refit_bvh.

    If the tree would be higher than PLOC_MAX_HEIGHT levels or needs more than PLOC_MAX_ITERATIONS iterations, the result is build_lbvh's tree (a rule of the
    specification, not an error).  `info`, when given, is filled with tree ("ploc" | "lbvh"), iterations and height (of the PLOC tree, None if it was not
    finished).  Same contract as build_lbvh: returns (nodes, perm), and upload_scene(nodes, tris[perm], mats) is the scene the form uploads."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    n = t.shape[0]
    if n == 0:
        raise ValueError("build_ploc: no triangles")
    keys = np.sort(lbvh_keys(t))
    perm = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    v = t[perm].reshape(-1, 4, 4)[:, :3, :3]
    with np.errstate(all="ignore"):
        lo, hi = np.fmin.reduce(v, axis=1), np.fmax.reduce(v, axis=1)  # a NaN coordinate takes no part (fminf / fmaxf)
    ids = np.arange(n, dtype=np.int64)  # provisional node of every cluster: < n a leaf (its sorted position), else inner node ids - n of `children`
    children = np.zeros((max(n - 1, 1), 2), dtype=np.int64)
    made, iterations = 0, 0
    if info is not None:
        info.update(tree="lbvh", iterations=None, height=None)
    while ids.size > 1:
        if iterations >= PLOC_MAX_ITERATIONS:
            return build_lbvh(t)
        iterations += 1
        m = ids.size
        nn = _ploc_nearest(lo, hi, radius)
        idx = np.arange(m, dtype=np.int64)
        mutual = nn[nn] == idx
        left = np.flatnonzero(mutual & (idx < nn))
        right = nn[left]
        new = n + made + np.arange(left.size, dtype=np.int64)
        children[new - n, 0], children[new - n, 1] = ids[left], ids[right]
        made += left.size
        with np.errstate(all="ignore"):
            lo[left], hi[left] = np.fmin(lo[left], lo[right]), np.fmax(hi[left], hi[right])
        ids[left] = new
        keep = np.ones(m, dtype=bool)
        keep[right] = False
        lo, hi, ids = lo[keep], hi[keep], ids[keep]
    if info is not None:
        info["iterations"] = iterations
    # the layout: level by level from the root, the children of the k-th inner node of a level at next_begin + 2 k, + 2 k + 1
    firsts, counts = [], []
    cur, next_index, height = ids[:1].copy(), 1, 0
    while cur.size:
        height += 1
        if height > PLOC_MAX_HEIGHT:
            return build_lbvh(t)
        inner = cur >= n
        first = cur.copy()
        k = int(inner.sum())
        first[inner] = next_index + 2 * np.arange(k, dtype=np.int64)
        firsts.append(first)
        counts.append(np.where(inner, 0, 1))
        next_index += 2 * k
        cur = children[cur[inner] - n].reshape(-1)
    if info is not None:
        info.update(tree="ploc", height=height)
    nodes = np.zeros(next_index, dtype=NODE_DTYPE)
    nodes["first"], nodes["count"] = np.concatenate(firsts), np.concatenate(counts)
    return refit_bvh(nodes, t[perm]), perm


SAH_BINS = 16           # == rv::kSahBins (rvpt_amd/csrc/rvpt_build.h) == kBins of bvh_builder.cpp
SAH_MIN_LEAF = 2        # == rv::kSahMinLeaf: below this a node is never split
SAH_MAX_LEAF = 8        # == rv::kSahMaxLeaf: above this a node is always split
SAH_BALANCE_DEPTH = 30  # == rv::kSahBalanceDepth: from this depth on only median splits

_FLT_MAX = np.float32(np.finfo(np.float32).max)


def _half_area(lo, hi):
    """float32 dx * (dy + dz) + dy * dz on extents clamped at 0 (bvh_builder.cpp: Box::half_area; a NaN extent stays a NaN, as std::max(NaN, 0) does)"""
    with np.errstate(all="ignore"):
        d = hi - lo
        d = np.where(d < 0, np.float32(0), d).astype(np.float32)
        return (d[..., 0] * (d[..., 1] + d[..., 2]) + d[..., 1] * d[..., 2]).astype(np.float32)


def _segment_min_max(lo_vals, hi_vals, starts):
    """exact min of lo_vals / max of hi_vals per contiguous non-empty segment; a NaN takes no part, an all-NaN segment gives +-FLT_MAX (the host's Box)"""
    with np.errstate(all="ignore"):
        lo = np.fmin.reduceat(np.where(np.isnan(lo_vals), _FLT_MAX, lo_vals), starts, axis=0)
        hi = np.fmax.reduceat(np.where(np.isnan(hi_vals), -_FLT_MAX, hi_vals), starts, axis=0)
    return np.minimum(lo, _FLT_MAX), np.maximum(hi, -_FLT_MAX)


def build_sah(tris, balance_depth: int = SAH_BALANCE_DEPTH):
    """The tree rvpt_hip_upload_scene's SAH BUILD FORM (RVPT_HIP_NODES_BUILD_SAH) makes on the device, in numpy — the second statement of "THE SAH TREE" in
    rvpt_amd/csrc/rvpt_build.h: rvpt_bvh_build's top-down binned-SAH build (bvh_builder.cpp: 16 bins per axis over the centroid bounds, leaves of 2 .. 8,
    traversal cost 0, median splits from depth 30 on) run level by level with every unstable step made stable.  Node for node it is the host builder's tree —
    the same triangle sets, the same boxes; only the order of triangles inside a leaf may differ (tests/test_sah_host.py).

    Per node (a range of the index array): exact bounds and centroid bounds; where depth < balance_depth, per axis 0, 1, 2 with extent > 0 the triangles are
    binned by f = (c - lo) * (16.0f / extent), bin = f >= 15 ? 15 : f >= 0 ? (int)f : 0, and the two sweeps of the host code pick the FIRST strict minimum of
    the cost in (axis, bin) order.  A binned split (cost < half_area(bounds) * count) is a STABLE partition by bin < best_bin; otherwise a node of <= 8 is a
    leaf; otherwise — and when a binned split leaves a side empty — the range is SORTED by (NaN last, centroid on the widest centroid axis with -0 == +0,
    caller's index) and cut at count / 2.  Layout as build_lbvh's: breadth first, the children of the k-th splitting node of a level at next_begin + 2 k.

    tris: float32[n, 16] in the CALLER'S order, n >= 1.  Returns (nodes, perm, info) with upload_scene(nodes, tris[perm], mats) the scene the form uploads and
    info = {height, binned_splits, median_splits, max_leaf}."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    n = t.shape[0]
    if n == 0:
        raise ValueError("build_sah: no triangles")
    v = t.reshape(-1, 4, 4)[:, :3, :3]
    third = np.float32(1.0) / np.float32(3.0)
    with np.errstate(all="ignore"):
        tlo, thi = np.fmin.reduce(v, axis=1), np.fmax.reduce(v, axis=1)  # a NaN coordinate takes no part (fminf / fmaxf)
        cent = (((v[:, 0] + v[:, 1]) + v[:, 2]) * third).astype(np.float32)  # float32, left to right
    idx = np.arange(n, dtype=np.int64)
    begin, count = np.zeros(1, dtype=np.int64), np.full(1, n, dtype=np.int64)
    firsts, counts = [], []
    next_index, depth = 1, 0
    info = {"height": 0, "binned_splits": 0, "median_splits": 0, "max_leaf": 0}
    max_height = 30 + int(np.ceil(np.log2(n))) + 1 if balance_depth == SAH_BALANCE_DEPTH else 64
    while begin.size:
        if depth >= max_height:
            raise ValueError(f"build_sah: the tree is higher than {max_height} levels")
        m = begin.size
        kind = np.zeros(m, dtype=np.int8)  # 0 leaf, 1 binned, 2 median
        n_left = np.zeros(m, dtype=np.int64)
        act = np.flatnonzero(count >= SAH_MIN_LEAF)
        if act.size:
            k = act.size
            cnt = count[act]
            starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            seg = np.repeat(np.arange(k, dtype=np.int64), cnt)
            pos = np.repeat(begin[act] - starts, cnt) + np.arange(seg.size, dtype=np.int64)  # positions of the index array, node after node
            ti = idx[pos]
            blo, bhi = _segment_min_max(tlo[ti], thi[ti], starts)
            clo, chi = _segment_min_max(cent[ti], cent[ti], starts)
            best_cost = np.full(k, _FLT_MAX, dtype=np.float32)
            best_axis = np.full(k, -1, dtype=np.int64)
            best_bin = np.zeros(k, dtype=np.int64)
            bins_of = np.zeros((3, seg.size), dtype=np.int64)
            with np.errstate(all="ignore"):
                ext = (chi - clo).astype(np.float32)
                scale = (np.float32(SAH_BINS) / ext).astype(np.float32)
                for ax in range(3 if depth < balance_depth else 0):
                    live = ext[:, ax] > 0
                    if not live.any():
                        continue
                    f = ((cent[ti, ax] - clo[seg, ax]) * scale[seg, ax]).astype(np.float32)
                    b = np.zeros(seg.size, dtype=np.int64)
                    inside = (f >= 0) & (f < SAH_BINS - 1)
                    b[inside] = f[inside].astype(np.int32)
                    b[f >= SAH_BINS - 1] = SAH_BINS - 1
                    bins_of[ax] = b
                    key = seg * SAH_BINS + b
                    order = np.argsort(key, kind="stable")
                    sk = key[order]
                    first_of = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
                    present = sk[first_of]
                    bin_lo = np.full((k * SAH_BINS, 3), _FLT_MAX, dtype=np.float32)
                    bin_hi = np.full((k * SAH_BINS, 3), -_FLT_MAX, dtype=np.float32)
                    bin_lo[present], bin_hi[present] = _segment_min_max(tlo[ti[order]], thi[ti[order]], first_of)
                    bin_cnt = np.bincount(key, minlength=k * SAH_BINS).astype(np.int64).reshape(k, SAH_BINS)
                    bin_lo, bin_hi = bin_lo.reshape(k, SAH_BINS, 3), bin_hi.reshape(k, SAH_BINS, 3)
                    right_cost = np.full((k, SAH_BINS), _FLT_MAX, dtype=np.float32)
                    alo, ahi = np.full((k, 3), _FLT_MAX, dtype=np.float32), np.full((k, 3), -_FLT_MAX, dtype=np.float32)
                    c = np.zeros(k, dtype=np.int64)
                    for bn in range(SAH_BINS - 1, 0, -1):
                        alo, ahi = np.minimum(alo, bin_lo[:, bn]), np.maximum(ahi, bin_hi[:, bn])
                        c = c + bin_cnt[:, bn]
                        right_cost[:, bn] = np.where(c > 0, (_half_area(alo, ahi) * c.astype(np.float32)).astype(np.float32), _FLT_MAX)
                    alo, ahi = np.full((k, 3), _FLT_MAX, dtype=np.float32), np.full((k, 3), -_FLT_MAX, dtype=np.float32)
                    c = np.zeros(k, dtype=np.int64)
                    for bn in range(SAH_BINS - 1):
                        alo, ahi = np.minimum(alo, bin_lo[:, bn]), np.maximum(ahi, bin_hi[:, bn])
                        c = c + bin_cnt[:, bn]
                        cost = ((_half_area(alo, ahi) * c.astype(np.float32)).astype(np.float32) + right_cost[:, bn + 1]).astype(np.float32)
                        better = live & (c > 0) & (right_cost[:, bn + 1] != _FLT_MAX) & (cost < best_cost)
                        best_cost = np.where(better, cost, best_cost)
                        best_axis = np.where(better, ax, best_axis)
                        best_bin = np.where(better, bn + 1, best_bin)
                leaf_cost = (_half_area(blo, bhi) * cnt.astype(np.float32)).astype(np.float32)
                binned = (best_axis >= 0) & (best_cost < leaf_cost)
            goes_left = np.zeros(seg.size, dtype=bool)
            if binned.any():
                goes_left = binned[seg] & (bins_of[np.maximum(best_axis, 0)[seg], np.arange(seg.size)] < best_bin[seg])
            nl = np.bincount(seg, weights=goes_left, minlength=k).astype(np.int64)
            binned &= (nl > 0) & (nl < cnt)  # a side left empty: the median split
            median = ~binned & ((cnt > SAH_MAX_LEAF) | ((best_axis >= 0) & (best_cost < leaf_cost)))
            kind[act] = np.where(binned, 1, np.where(median, 2, 0))
            n_left[act] = np.where(binned, nl, cnt // 2)
            # the widest centroid axis: the first strict maximum, from -1
            with np.errstate(all="ignore"):
                widest, m_axis = np.full(k, -1.0, dtype=np.float32), np.zeros(k, dtype=np.int64)
                for ax in range(3):
                    w = ext[:, ax] > widest
                    widest, m_axis = np.where(w, ext[:, ax], widest), np.where(w, ax, m_axis)
            # one stable sort of every position of a splitting node: binned nodes by (node, goes right), median nodes by (node, NaN, value, index)
            split_pos = binned[seg] | median[seg]
            if split_pos.any():
                sp = np.flatnonzero(split_pos)
                s_seg, s_ti = seg[sp], ti[sp]
                val = cent[s_ti, m_axis[s_seg]]
                is_nan = np.isnan(val)
                med = median[s_seg]
                with np.errstate(all="ignore"):
                    k1 = np.where(med, is_nan.astype(np.int64), (~goes_left[sp]).astype(np.int64))
                    k2 = np.where(med & ~is_nan, val + np.float32(0), np.float32(0))  # -0 + 0 = +0
                    k3 = np.where(med, s_ti, 0)
                order = np.lexsort((k3, k2, k1, s_seg))  # stable: equal keys keep their order
                idx[pos[sp]] = s_ti[order]
        leaf = kind == 0
        info["binned_splits"] += int((kind == 1).sum())
        info["median_splits"] += int((kind == 2).sum())
        if leaf.any():
            info["max_leaf"] = max(info["max_leaf"], int(count[leaf].max()))
        n_split = int((~leaf).sum())
        first = begin.copy()
        first[~leaf] = next_index + 2 * np.arange(n_split, dtype=np.int64)
        firsts.append(first)
        counts.append(np.where(leaf, count, 0))
        next_index += 2 * n_split
        sb, sc, sl = begin[~leaf], count[~leaf], n_left[~leaf]
        begin = np.stack([sb, sb + sl], axis=1).reshape(-1)
        count = np.stack([sl, sc - sl], axis=1).reshape(-1)
        depth += 1
    info["height"] = depth
    perm = idx.astype(np.uint32)
    nodes = np.zeros(next_index, dtype=NODE_DTYPE)
    nodes["first"], nodes["count"] = np.concatenate(firsts), np.concatenate(counts)
    return refit_bvh(nodes, t[perm]), perm, info


def wobble(tris, phase: float, amplitude: float) -> np.ndarray:
    """A smooth deformation for moving-geometry demos, tests and tools/refit_bench.py: every vertex is displaced by a function of its own position and `phase`
    alone (three sines of the other two coordinates), so vertices that coincide stay welded; |displacement| <= amplitude * sqrt(3).  The .w lanes and the
    material row are kept.  float32[n, 16] -> float32[n, 16]."""
    t = np.array(tris, dtype=np.float32).reshape(-1, 16)
    p = t.reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    ext = float(np.ptp(p.reshape(-1, 3), axis=0).max()) or 1.0
    k = 2.0 * np.pi / ext
    d = np.stack([np.sin(1.3 * k * p[..., 1] + 0.7 * k * p[..., 2] + phase), np.sin(0.9 * k * p[..., 2] + 1.1 * k * p[..., 0] + 1.7 * phase),
                  np.sin(1.2 * k * p[..., 0] + 0.8 * k * p[..., 1] + 2.3 * phase)], axis=-1)
    t.reshape(-1, 4, 4)[:, :3, :3] = (p + amplitude * d).astype(np.float32)
    return t


PART_MOVE_DTYPE = np.dtype([("m", "<f4", (12,)), ("first", "<u4"), ("count", "<u4"), ("reserved", "<u4", (2,))])  # rvpt_part_move (== native.PART_MOVE_DTYPE)


def part_moves(moves) -> np.ndarray:
    """A list of moves as PART_MOVE_DTYPE records: a structured array of that dtype as it is, or a sequence of (first, count, matrix) with a 3x4 matrix or a
    4x4 matrix whose last row is 0 0 0 1.  Raises ValueError for anything else: a negative `first` or `count`, one past 2^32 - 1, a matrix of another shape."""
    if isinstance(moves, np.ndarray) and moves.dtype == PART_MOVE_DTYPE:
        return np.ascontiguousarray(moves).reshape(-1)
    out = np.zeros(len(moves), dtype=PART_MOVE_DTYPE)
    for p, move in enumerate(moves):
        if isinstance(move, np.void) and move.dtype == PART_MOVE_DTYPE:  # (a record among tuples, part_move's say)
            out[p] = move
            continue
        first, count, matrix = move
        first, count = int(first), int(count)
        if not 0 <= first <= 0xFFFFFFFF or not 0 <= count <= 0xFFFFFFFF:
            raise ValueError(f"moves[{p}]: first = {first}, count = {count} is not a range of triangles")
        m = np.asarray(matrix, dtype=np.float32)
        if m.shape == (4, 4):
            if m[3].tobytes() != np.array([0, 0, 0, 1], dtype=np.float32).tobytes():
                raise ValueError(f"moves[{p}]: the last row of a 4x4 matrix must be 0 0 0 1, got {m[3].tolist()}")
            m = m[:3]
        if m.shape != (3, 4):
            raise ValueError(f"moves[{p}]: the matrix is 3x4 or 4x4, got {m.shape}")
        out[p] = (m.reshape(12), first, count, (0, 0))
    return out


def part_move(first: int, count: int, rotation=None, translation=None) -> np.ndarray:
    """One rvpt_part_move row from a rotation (3x3, None: the identity) and a translation (3, None: none): x' = R x + t, rounded to float32."""
    m = np.zeros((3, 4), dtype=np.float32)
    m[:, :3] = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
    if translation is not None:
        m[:, 3] = np.asarray(translation, dtype=np.float64).reshape(3)
    return part_moves([(first, count, m)])[0]


def pose_parts(rest_tris, moves, current=None) -> np.ndarray:
    """The normative statement of the POSE UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): the triangles [first, first + count) of every move are posed FROM
    `rest_tris` by the move's 3x4 matrix; every other row is `current`'s (None: rest_tris').  Per vertex and output component i the value is
    ((m[4i]*x + m[4i+1]*y) + m[4i+2]*z) + m[4i+3] in float32: three products and three sums, each rounded on its own — numpy never fuses — so the device and the
    host give the same bits.  Only x, y, z of the three vertices change: the .w lanes are the rest pose's, the material row is `current`'s.
    moves: what part_moves takes.  The ranges must lie inside the array and share no triangle (ValueError).  float32[n, 16] -> a new float32[n, 16]."""
    rest = np.ascontiguousarray(rest_tris, dtype=np.float32).reshape(-1, 16)
    out = rest.copy() if current is None else np.array(current, dtype=np.float32).reshape(-1, 16)
    if out.shape != rest.shape:
        raise ValueError(f"pose_parts: current has {out.shape[0]} triangles, the rest pose {rest.shape[0]}")
    rec = part_moves(moves)
    taken = np.zeros(rest.shape[0], dtype=bool)
    for p, r in enumerate(rec):
        first, count = int(r["first"]), int(r["count"])
        if first + count > rest.shape[0]:
            raise ValueError(f"pose_parts: moves[{p}] = [{first}, {first} + {count}) is outside the {rest.shape[0]} triangles")
        if taken[first:first + count].any():
            raise ValueError(f"pose_parts: moves[{p}] shares triangle {first + int(np.argmax(taken[first:first + count]))} with an earlier move")
        taken[first:first + count] = True
        m = r["m"].reshape(3, 4)
        v = rest[first:first + count].reshape(-1, 4, 4)[:, :3, :]  # [count, vertex, xyzw]
        x, y, z = v[..., 0:1], v[..., 1:2], v[..., 2:3]
        with np.errstate(all="ignore"):
            xyz = ((m[:, 0] * x + m[:, 1] * y) + m[:, 2] * z) + m[:, 3]  # float32 throughout: [count, vertex, i]
        rows = out[first:first + count].reshape(-1, 4, 4)
        rows[:, :3, :3] = xyz
        rows[:, :3, 3] = v[..., 3]
        out[first:first + count] = rows.reshape(-1, 16)
    return out


VERTEX_SKIN_DTYPE = np.dtype([("bone", "<u4", (4,)), ("weight", "<f4", (4,))])  # rvpt_vertex_skin (== native.VERTEX_SKIN_DTYPE)
SKIN_MAX_BONES = 1024  # == RVPT_HIP_SKIN_MAX_BONES


def vertex_skins(skin, weights=None) -> np.ndarray:
    """The four influences of every vertex as VERTEX_SKIN_DTYPE records [3 n], record 3 t + v for vertex v of triangle t: a structured array of that dtype as it
    is (any shape of 3 n records), or the pair (indices[n, 3, 4], weights[n, 3, 4]) — as two arguments or as one tuple.  Raises ValueError for anything else:
    another shape, a record count that is no multiple of three, indices that are not integers, a negative index or one past 2^32 - 1."""
    if weights is None and isinstance(skin, (tuple, list)) and len(skin) == 2:
        skin, weights = skin
    if weights is None:
        if not (isinstance(skin, np.ndarray) and skin.dtype == VERTEX_SKIN_DTYPE):
            raise ValueError("vertex_skins: a VERTEX_SKIN_DTYPE array or a pair (indices[n, 3, 4], weights[n, 3, 4]) is needed")
        rec = np.ascontiguousarray(skin).reshape(-1)
        if rec.shape[0] % 3:
            raise ValueError(f"vertex_skins: {rec.shape[0]} records are not three per triangle")
        return rec
    idx, w = np.asarray(skin), np.asarray(weights)
    if idx.ndim != 3 or idx.shape[1:] != (3, 4) or w.shape != idx.shape:
        raise ValueError(f"vertex_skins: indices and weights are [n, 3, 4] both, got {idx.shape} and {w.shape}")
    if idx.size and not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"vertex_skins: the indices are integers, got {idx.dtype}")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) > 0xFFFFFFFF):
        bad = int(np.flatnonzero((idx.reshape(-1) < 0) | (idx.reshape(-1) > 0xFFFFFFFF))[0])
        raise ValueError(f"vertex_skins: skin[{bad // 4}].bone[{bad % 4}] = {int(idx.reshape(-1)[bad])} is not a bone index")
    rec = np.zeros(idx.shape[0] * 3, dtype=VERTEX_SKIN_DTYPE)
    rec["bone"] = idx.reshape(-1, 4).astype(np.uint32)
    rec["weight"] = w.reshape(-1, 4).astype(np.float32)
    return rec


def bone_matrices(bones) -> np.ndarray:
    """The matrices of a skin update as float32[k, 12] (rvpt_bone: 3x4, row major): float32[k, 3, 4] or [k, 12] as they are, or [k, 4, 4] with every last row
    0 0 0 1.  ValueError for another shape, such a last row, or more than SKIN_MAX_BONES matrices."""
    m = np.asarray(bones, dtype=np.float32)
    if m.ndim == 3 and m.shape[1:] == (4, 4):
        last = np.array([0, 0, 0, 1], dtype=np.float32)
        bad = np.flatnonzero((m[:, 3].view(np.uint32) != last.view(np.uint32)).any(axis=1))
        if bad.size:
            raise ValueError(f"bones[{int(bad[0])}]: the last row of a 4x4 matrix must be 0 0 0 1, got {m[int(bad[0]), 3].tolist()}")
        m = m[:, :3]
    if not ((m.ndim == 3 and m.shape[1:] == (3, 4)) or (m.ndim == 2 and m.shape[1] == 12)):
        raise ValueError(f"bones: float32[k, 3, 4], [k, 12] or [k, 4, 4] is needed, got {m.shape}")
    if m.shape[0] > SKIN_MAX_BONES:
        raise ValueError(f"bones: {m.shape[0]} matrices, at most {SKIN_MAX_BONES}")
    return np.ascontiguousarray(m.reshape(-1, 12))


def skin_triangles(rest_tris, skin, bones) -> np.ndarray:
    """The normative statement of the SKIN UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): linear blend skinning of EVERY vertex of `rest_tris`.  For a
    vertex p with the record (bone[4], weight[4]): q_j = ((m0 x + m1 y) + m2 z) + m3 per component with the matrix of bone[j] — pose_parts' arithmetic —, then
    out_i = ((w0 q0_i + w1 q1_i) + w2 q2_i) + w3 q3_i: float32 throughout, every product and sum rounded on its own (numpy never fuses), all four influences
    always evaluated, so the device and the host give the same bits.  Only x, y, z of the three vertices change: the .w lanes and the material row are kept.
    skin: what vertex_skins takes, in the triangles' order; bones: what bone_matrices takes.  ValueError for a shape mismatch, a bone index >= len(bones), or more
    than SKIN_MAX_BONES bones.  float32[n, 16] -> a new float32[n, 16]."""
    rest = np.ascontiguousarray(rest_tris, dtype=np.float32).reshape(-1, 16)
    rec = vertex_skins(skin)
    m = bone_matrices(bones).reshape(-1, 3, 4)
    if rec.shape[0] != 3 * rest.shape[0]:
        raise ValueError(f"skin_triangles: {rec.shape[0]} records for {rest.shape[0]} triangles: three per triangle")
    if rec.size and int(rec["bone"].max()) >= m.shape[0]:
        r, j = np.argwhere(rec["bone"] >= m.shape[0])[0]
        raise ValueError(f"skin_triangles: skin[{int(r)}].bone[{int(j)}] = {int(rec['bone'][r, j])} with {m.shape[0]} bones")
    out = rest.copy()
    v = rest.reshape(-1, 4, 4)[:, :3, :].reshape(-1, 4)  # [3 n, xyzw]
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    with np.errstate(all="ignore"):
        q = []
        for j in range(4):
            mj = m[rec["bone"][:, j]]  # [3 n, 3, 4]
            q.append(((mj[:, :, 0] * x + mj[:, :, 1] * y) + mj[:, :, 2] * z) + mj[:, :, 3])  # [3 n, i]
        w = rec["weight"]
        xyz = ((w[:, 0:1] * q[0] + w[:, 1:2] * q[1]) + w[:, 2:3] * q[2]) + w[:, 3:4] * q[3]
    assert xyz.dtype == np.float32
    out.reshape(-1, 4, 4)[:, :3, :3] = xyz.reshape(-1, 3, 3)
    return out


POINT_HIT_DTYPE = np.dtype([("point", "<f4", (3,)), ("max_d2", "<f4"), ("closest", "<f4", (3,)), ("d2", "<f4"), ("prim", "<u4"), ("u", "<f4"), ("v", "<f4"),
                            ("region", "<u4")])  # rvpt_point_hit (== native.POINT_HIT_DTYPE)
NO_PRIM = 0xFFFFFFFF  # a record's prim after a miss


def _dot_rounded(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _quotient(num, den):
    """The correctly rounded float32 quotient; a quotient whose divisor is 0 is taken as 0."""
    zero = den == 0
    return np.where(zero, np.float32(0), num / np.where(zero, np.float32(1), den)).astype(np.float32)


def closest_point_triangles(p, tris):
    """The per-triangle arithmetic of a POINT QUERY (include/rvpt_hip.h: NEAREST POINTS), vectorised: the candidate of every triangle of `tris` (float32[n, 16]
    rows, or [n, 3, 3] vertices) for every point of `p` (float32[3] or [m, 3]).  float32 throughout, every product, sum and quotient rounded on its own — numpy
    never fuses, and its float32 divide is the correctly rounded one — so the device and the host give the same bits: Ericson's point-triangle test with its
    regions tested in the header's order (the first that holds decides u, v, region), q = (a + ab*u) + ac*v clamped into the triangle's own box by comparisons
    that leave a NaN a NaN, d2 = (dx*dx + dy*dy) + dz*dz with d = p - q.
    Returns (closest[..., n, 3], d2[..., n], u[..., n], v[..., n], region[..., n] uint32), the leading axis being p's (none for a single point)."""
    t = np.asarray(tris, dtype=np.float32)
    verts = t.reshape(-1, 4, 4)[:, :3, :3] if t.ndim == 2 and t.shape[1] == 16 else t.reshape(-1, 3, 3)
    p = np.asarray(p, dtype=np.float32)
    single = p.ndim == 1
    q, dist2, u, v, region = _closest_point_pairs(p.reshape(-1, 1, 3), verts)  # [m, 1, 3] against [n, 3]
    if single:
        return q[0], dist2[0], u[0], v[0], region[0]
    return q, dist2, u, v, region


def _closest_point_pairs(pp, verts):
    """closest_point_triangles' arithmetic for points pp[m, 1 or n, 3] against the vertices verts[n, 3, 3]: one point per row, or one per (row, triangle) pair."""
    a, b, c = verts[:, 0], verts[:, 1], verts[:, 2]
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = pp - a, pp - b, pp - c
        ab_, ac_ = np.broadcast_to(ab, ap.shape), np.broadcast_to(ac, ap.shape)
        d1, d2, d3, d4, d5, d6 = _dot_rounded(ab_, ap), _dot_rounded(ac_, ap), _dot_rounded(ab_, bp), _dot_rounded(ac_, bp), _dot_rounded(ab_, cp), _dot_rounded(ac_, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e1, e2 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (e1 >= 0) & (e2 >= 0)]
        region = np.select(conds, [1, 2, 4, 3, 5, 6], default=0).astype(np.uint32)  # (np.select takes the first condition that holds)
        s = (va + vb) + vc
        w = _quotient(e1, e1 + e2)
        u = np.select([region == 2, region == 4, region == 6, region == 0], [np.broadcast_to(one, s.shape), _quotient(d1, d1 - d3), one - w, _quotient(vb, s)], default=zero)
        v = np.select([region == 3, region == 5, region == 6, region == 0], [np.broadcast_to(one, s.shape), _quotient(d2, d2 - d6), w, _quotient(vc, s)], default=zero)
        u, v = u.astype(np.float32), v.astype(np.float32)
        q = (a + ab * u[..., None]) + ac * v[..., None]
        lo, hi = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
        q = np.where(q < lo, lo, np.where(q > hi, hi, q))
        d = pp - q
        dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert q.dtype == np.float32 and dist2.dtype == np.float32
    return q, dist2, u, v, region


def point_box_d2(p, lo, hi):
    """The squared distance from p[..., 3] to the boxes [lo, hi] as a point query's walk computes it: g = max(max(lo - p, p - hi), 0) per axis, then
    (gx*gx + gy*gy) + gz*gz in float32 — the expression shape of closest_point_triangles' d2, which is what makes box_d2 <= d2 hold in floats for every triangle
    inside the box."""
    p, lo, hi = np.asarray(p, dtype=np.float32), np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    with np.errstate(all="ignore"):
        g = np.fmax(np.fmax(lo - p, p - hi), np.float32(0))
        return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def closest_points(tris, points, max_d2=np.inf, chunk: int = 1 << 20) -> np.ndarray:
    """The normative statement of a POINT QUERY (include/rvpt_hip.h: NEAREST POINTS), by brute force: every triangle's candidate (d2_i, i) from
    closest_point_triangles, the answer the lexicographically smallest one below (max_d2, 0xFFFFFFFF) — a NaN d2 never wins, d2 == max_d2 is accepted, among
    equal d2 the smaller index.  `tris` (float32[n, 16]) in the order the update form takes on the context asked, which is the numbering of prim; points
    float32[m, 3]; max_d2 a scalar or one SQUARED bound per point.  A point with a non-finite component, a max_d2 that is NaN or < 0, and a miss go out as
    closest 0, d2 = the bits of max_d2, prim NO_PRIM, u = v = 0, region 0.  Returns POINT_HIT_DTYPE[m] with the in fields filled."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    rec = np.zeros(pts.shape[0], dtype=POINT_HIT_DTYPE)
    rec["point"] = pts
    rec["max_d2"] = np.asarray(max_d2, dtype=np.float32)
    rec["d2"], rec["prim"] = rec["max_d2"], NO_PRIM
    bound = rec["max_d2"]
    with np.errstate(all="ignore"):
        valid = np.isfinite(pts).all(axis=1) & (bound >= 0)
    rows = np.flatnonzero(valid)
    n = t.shape[0]
    if n == 0 or rows.size == 0:
        return rec
    step = max(1, chunk // n)
    for lo in range(0, rows.size, step):
        sel = rows[lo:lo + step]
        q, d2, u, v, region = closest_point_triangles(pts[sel], t)
        with np.errstate(all="ignore"):
            ok = d2 <= bound[sel, None]  # (false for a NaN d2)
        key = np.where(ok, d2, np.float32(np.inf))
        best = ok & (key == key.min(axis=1, keepdims=True))
        hit = best.any(axis=1)
        i = np.argmax(best, axis=1)  # the first, hence the smallest index among equal d2
        k = np.arange(sel.size)
        out = rec[sel]
        out["closest"][hit], out["d2"][hit] = q[k, i][hit], d2[k, i][hit]
        out["prim"][hit], out["u"][hit], out["v"][hit], out["region"][hit] = i[hit].astype(np.uint32), u[k, i][hit], v[k, i][hit], region[k, i][hit]
        rec[sel] = out
    return rec


POINT_MAX_NEAREST = 8  # == RVPT_HIP_POINT_MAX_NEAREST


def closest_points_k(tris, points, k: int, max_d2=np.inf, chunk: int = 1 << 20) -> np.ndarray:
    """The normative statement of a K-NEAREST POINT QUERY (include/rvpt_hip.h: K-NEAREST POINTS), by brute force: closest_points' candidates (d2_i, i), every
    one of them, from closest_point_triangles; the answer of a point is the first k, in ascending lexicographic order of (d2, i), of the candidates below
    (max_d2, 0xFFFFFFFF) — a stable sort by d2 of the accepted candidates in index order, a NaN d2 excluded, d2 == max_d2 accepted.  Arguments as for
    closest_points; k = 1 .. POINT_MAX_NEAREST.  Returns POINT_HIT_DTYPE[m, k]: column j holds the j-th entry; from the first slot no candidate fills, and in
    every slot of a point that closest_points calls invalid, the miss (closest 0, d2 = the bits of the point's max_d2, prim NO_PRIM, u = v = 0, region 0).
    The in fields are filled in column 0 only (a query ignores the followers'), so column 0 is closest_points' answer, byte for byte."""
    k = int(k)
    if not 1 <= k <= POINT_MAX_NEAREST:
        raise ValueError(f"k must be 1 .. {POINT_MAX_NEAREST}, got {k}")
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    m = pts.shape[0]
    rec = np.zeros((m, k), dtype=POINT_HIT_DTYPE)
    rec["point"][:, 0] = pts
    rec["max_d2"][:, 0] = np.asarray(max_d2, dtype=np.float32)
    bound = rec["max_d2"][:, 0].copy()
    rec["d2"], rec["prim"] = bound[:, None], NO_PRIM
    with np.errstate(all="ignore"):
        valid = np.isfinite(pts).all(axis=1) & (bound >= 0)
    rows = np.flatnonzero(valid)
    n = t.shape[0]
    if n == 0 or rows.size == 0:
        return rec
    step = max(1, chunk // n)
    take = min(k, n)
    for lo in range(0, rows.size, step):
        sel = rows[lo:lo + step]
        q, d2, u, v, region = closest_point_triangles(pts[sel], t)
        with np.errstate(all="ignore"):
            ok = d2 <= bound[sel, None]  # (false for a NaN d2)
        # a stable sort of the keys with the refused ones last: a key of +inf may be an accepted candidate (max_d2 = +inf), so the refused sort on a flag first
        order = np.lexsort((d2, ~ok), axis=1)[:, :take]  # (lexsort is stable: equal (flag, d2) keep index order)
        r = np.arange(sel.size)[:, None]
        filled = ok[r, order]
        out = rec[sel]
        for name, src in (("closest", q), ("d2", d2), ("u", u), ("v", v), ("region", region)):
            dst = out[name][:, :take]
            dst[filled] = src[r, order][filled]
        out["prim"][:, :take][filled] = order[filled].astype(np.uint32)
        rec[sel] = out
    return rec


BOX_OVERLAP_DTYPE = np.dtype([("lo", "<f4", (3,)), ("prim_from", "<u4"), ("hi", "<f4", (3,)), ("flags", "<u4"), ("count", "<u4"),
                              ("prim", "<u4", (3,))])  # rvpt_box_overlap (== native.BOX_OVERLAP_DTYPE)
BOX_MAX_GROUP = 4  # == RVPT_HIP_BOX_MAX_GROUP


def triangle_box_overlaps(tris, lo, hi) -> np.ndarray:
    """THE TEST of a BOX QUERY (include/rvpt_hip.h: BOX OVERLAPS), vectorised: which triangles of `tris` (float32[n, 16] rows, or [n, 3, 3] vertices) meet the
    closed boxes [lo, hi] (float32[3] or [m, 3] each).  The rounded separating-axis test over 13 axes, every operation in np.float32 and rounded on its own (numpy
    never fuses); every comparison is a rejection — "min(p) > r" is written as all three above r — so a NaN rejects nothing; a triangle with a non-finite vertex
    component never passes.  The boxes are taken as they are: whether a record is valid is box_overlaps' business.  Returns bool[m, n] (bool[n] for one box)."""
    t = np.asarray(tris, dtype=np.float32)
    verts = t.reshape(-1, 4, 4)[:, :3, :3] if t.ndim == 2 and t.shape[1] == 16 else t.reshape(-1, 3, 3)
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    single = lo.ndim == 1
    lo, hi = lo.reshape(-1, 1, 3), hi.reshape(-1, 1, 3)  # [m, 1, 3] against [n, 3]
    a, b, c = verts[:, 0], verts[:, 1], verts[:, 2]
    half = np.float32(0.5)
    with np.errstate(all="ignore"):
        finite = np.isfinite(verts).all(axis=(1, 2))
        # 1. boxes: comparisons only
        apart = (((a > hi) & (b > hi) & (c > hi)) | ((a < lo) & (b < lo) & (c < lo))).any(axis=-1)
        # 2. set-up
        ctr = lo * half + hi * half
        h = hi - ctr
        v = [a - ctr, b - ctr, c - ctr]
        e = [b - a, c - b, a - c]
        # 3. the plane
        x, y = b - a, c - a
        n = np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=-1)
        up = n > 0
        vmin, vmax = np.where(up, -h - v[0], h - v[0]), np.where(up, h - v[0], -h - v[0])
        n_ = np.broadcast_to(n, vmin.shape)
        apart = apart | (_dot_rounded(n_, vmin) > 0) | (_dot_rounded(n_, vmax) < 0)
        # 4. the nine edge axes
        for ei in e:
            for j in range(3):
                k1, k2 = (j + 1) % 3, (j + 2) % 3
                p = [ei[:, k1] * vm[..., k2] - ei[:, k2] * vm[..., k1] for vm in v]
                r = h[..., k1] * np.abs(ei[:, k2]) + h[..., k2] * np.abs(ei[:, k1])
                assert p[0].dtype == np.float32 and r.dtype == np.float32
                apart = apart | ((p[0] > r) & (p[1] > r) & (p[2] > r)) | ((p[0] < -r) & (p[1] < -r) & (p[2] < -r))
    meets = finite & ~apart
    return meets[0] if single else meets


def box_overlaps(tris, records, k: int = 1, perm=None, chunk: int = 1 << 22) -> np.ndarray:
    """The normative statement of a BOX QUERY (include/rvpt_hip.h: BOX OVERLAPS), by brute force.  `records` holds n groups of k BOX_OVERLAP_DTYPE records (flat
    or [n, k]); record 0 of a group carries the box and prim_from.  A is every triangle of `tris` (float32[m, 16], stored order) that passes
    triangle_box_overlaps and whose reported number — its index, or perm[index] with a permutation — is >= prim_from; count = |A| goes to record 0's count, the
    4k - 1 smallest reported numbers, ascending, to the prim slots of record 0 and then to the whole out quads of records 1 .. k - 1, 0xFFFFFFFF from the first
    slot A does not fill.  A record 0 with a non-finite corner or lo > hi on some axis, and every record of the empty scene, gets count 0 and every slot
    0xFFFFFFFF.  Returns a copy of `records`, same shape, with the out quads written and every in quad — the followers' included — as it came."""
    k = int(k)
    if not 1 <= k <= BOX_MAX_GROUP:
        raise ValueError(f"k must be 1 .. {BOX_MAX_GROUP}, got {k}")
    rec = np.asarray(records)
    if rec.dtype != BOX_OVERLAP_DTYPE or rec.size % k:
        raise ValueError(f"box_overlaps: BOX_OVERLAP_DTYPE records in groups of {k} are needed, got {rec.dtype} x {rec.size}")
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    out = np.ascontiguousarray(rec).copy()
    g = out.reshape(-1, k)
    n, m, slots = g.shape[0], t.shape[0], 4 * k - 1
    number = np.arange(m, dtype=np.uint32) if perm is None else np.asarray(perm, dtype=np.uint32).reshape(m)
    lo, hi, prim_from = g["lo"][:, 0], g["hi"][:, 0], g["prim_from"][:, 0]
    with np.errstate(all="ignore"):
        valid = np.isfinite(lo).all(axis=1) & np.isfinite(hi).all(axis=1) & (lo <= hi).all(axis=1)
    quads = np.full((n, 4 * k), NO_PRIM, dtype=np.uint32)
    quads[:, 0] = 0
    rows = np.flatnonzero(valid)
    order = np.argsort(number, kind="stable")
    step = max(1, chunk // max(m, 1))
    for at in range(0, rows.size if m else 0, step):
        sel = rows[at:at + step]
        member = triangle_box_overlaps(t, lo[sel], hi[sel]) & (number[None, :] >= prim_from[sel, None])
        quads[sel, 0] = member.sum(axis=1)
        by_number = member[:, order]  # columns in ascending reported number
        for row, box in enumerate(sel):
            listed = number[order[np.flatnonzero(by_number[row])[:slots]]]
            quads[box, 1:1 + listed.size] = listed
    out.view(np.uint32).reshape(n, k, 12)[:, :, 8:] = quads.reshape(n, k, 4)
    return out


SPHERE_SWEEP_DTYPE = np.dtype([("org", "<f4", (3,)), ("radius", "<f4"), ("dir", "<f4", (3,)), ("tmax", "<f4"), ("t", "<f4"), ("prim", "<u4"), ("u", "<f4"),
                               ("v", "<f4")])  # rvpt_sphere_sweep (== native.SPHERE_SWEEP_DTYPE)
SWEEP_FEATURES = ("face", "vertex a", "vertex b", "vertex c", "edge ab", "edge bc", "edge ca")  # the columns of sweep_feature_times


def sweep_slab(p, d, r, tmax, lo, hi):
    """Step 1 of a SPHERE SWEEP (include/rvpt_hip.h: SPHERE SWEEPS): the centre's path p + t*d, t in [0, tmax], against the box [lo, hi] inflated by one rounded
    operation per side, L = lo - r and H = hi + r.  p, d, lo, hi [..., 3], r and tmax [...], broadcast against each other; float32 throughout.  Per axis with
    d == 0 the two comparisons p < L, p > H reject and nothing else happens; otherwise inv = 1/d, t1 = (L - p)*inv, t2 = (H - p)*inv, near and far are t1 and t2
    by the sign of d, and t_in = near > t_in ? near : t_in from 0, t_out = far < t_out ? far : t_out from tmax — selects, so that a NaN changes nothing.  Passes
    iff nothing rejected, t_in <= t_out and t_in < +inf.  Every operation is monotone in lo and hi, which is the pruning lemma.  Returns (passes, t_in)."""
    f32 = np.float32
    p, d, lo, hi = (np.asarray(x, dtype=f32) for x in (p, d, lo, hi))
    r, tmax = np.asarray(r, dtype=f32), np.asarray(tmax, dtype=f32)
    with np.errstate(all="ignore"):
        low, high = lo - r[..., None], hi + r[..., None]
        zero = d == 0
        inv = f32(1) / np.where(zero, f32(1), d)
        t1, t2 = (low - p) * inv, (high - p) * inv
        near, far = np.where(d > 0, t1, t2), np.where(d > 0, t2, t1)
        outside = (zero & ((p < low) | (p > high))).any(axis=-1)
        shape = np.broadcast(outside, tmax).shape
        t_in, t_out = np.zeros(shape, dtype=f32), np.broadcast_to(tmax, shape).astype(f32)
        for k in range(3):
            nk, fk = np.where(zero[..., k], f32(-np.inf), near[..., k]), np.where(zero[..., k], f32(np.inf), far[..., k])
            t_in = np.where(nk > t_in, nk, t_in)
            t_out = np.where(fk < t_out, fk, t_out)
        passes = ~outside & (t_in <= t_out) & (t_in < f32(np.inf))
    assert t_in.dtype == f32
    return passes, t_in


def _cross_rounded(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2], x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def sweep_feature_times(p, d, r, tmax, verts):
    """Step 2 of a SPHERE SWEEP: the contact time of each of the seven features of every triangle verts[n, 3, 3] for the records p, d [m, 3], r, tmax [m],
    float32 [m, n, 7] in the order of SWEEP_FEATURES, +inf where a feature has none.  Every accepted time is a number in [0, tmax]."""
    f32 = np.float32
    inf, zero = f32(np.inf), f32(0)
    pp, dd = p[:, None, :], d[:, None, :]
    rr, big_t = (r * r)[:, None], tmax[:, None]
    a, b, c = verts[:, 0], verts[:, 1], verts[:, 2]
    shape = (p.shape[0], verts.shape[0])
    out = np.full(shape + (7,), inf, dtype=f32)
    big_a = np.broadcast_to(_dot_rounded(dd, dd), shape)

    def root(c0, b0, a0, gate):  # the smaller root of a0*t*t + 2*b0*t + c0 as c0 / (sqrt(b0*b0 - a0*c0) - b0), where the centre starts outside and approaches
        disc = b0 * b0 - a0 * c0
        ok = gate & (c0 > 0) & (b0 < 0) & (a0 > 0) & (disc >= 0)
        t = c0 / np.where(ok, np.sqrt(np.where(ok, disc, zero)) - b0, f32(1))
        return t, ok & (t >= 0) & (t <= big_t)

    for k, (x0, x1) in enumerate(((a, b), (b, c), (c, a))):
        m = pp - x0
        dm = np.broadcast_to(dd, m.shape)
        big_b, big_c = _dot_rounded(m, dm), _dot_rounded(m, m) - rr
        t, ok = root(big_c, big_b, big_a, True)
        out[..., 1 + k] = np.where(big_c <= 0, zero, np.where(ok, t, inf))
        e = np.broadcast_to(x1 - x0, m.shape)
        ee, md, nd = _dot_rounded(e, e), _dot_rounded(m, e), _dot_rounded(dm, e)
        ca, cb, cc = ee * big_a - nd * nd, ee * big_b - nd * md, ee * big_c - md * md
        t, ok = root(cc, cb, ca, ee > 0)
        s = md + t * nd
        ok = ok & (s >= 0) & (s <= ee)
        inside = (ee > 0) & (cc <= 0) & (md >= 0) & (md <= ee)
        out[..., 4 + k] = np.where(inside, zero, np.where(ok, t, inf))
    n = _cross_rounded(b - a, c - a)
    nn = _dot_rounded(n, n)
    m = pp - a
    h = _dot_rounded(m, np.broadcast_to(n, m.shape))
    rn = r[:, None] * np.sqrt(nn)
    hs, dn = np.abs(h), _dot_rounded(np.broadcast_to(dd, m.shape), np.broadcast_to(n, m.shape))
    dns = np.where(h > 0, dn, -dn)
    within = hs <= rn
    moving = ~within & (hs > rn) & (dns < 0)
    t = np.where(within, zero, (rn - hs) / np.where(moving, dns, f32(1)))
    ok = (nn > 0) & (within | (moving & (t >= 0) & (t <= big_t)))
    t = np.where(ok, t, zero)
    centre = pp + dd * t[..., None]
    region = _closest_point_pairs(centre, verts)[4]
    out[..., 0] = np.where(ok & (region == 0), t, inf)
    assert out.dtype == f32
    return out


def sweep_sphere_triangles(org, direction, radius, tmax, tris):
    """The per-triangle arithmetic of a SPHERE SWEEP (include/rvpt_hip.h: SPHERE SWEEPS), vectorised: the candidate of every triangle of `tris` (float32[n, 16]
    rows, or [n, 3, 3] vertices) for one record (org[3], direction[3], radius, tmax) or for m of them ([m, 3], [m, 3], [m], [m]).  float32 throughout, every
    product, sum, quotient and square root rounded on its own, in the header's order: the own box's slab test (sweep_slab) gives t_in, the seven features
    (sweep_feature_times) give t_tri as their smallest time, t = t_in > t_tri ? t_in : t_tri, and (u, v) are closest_point_triangles' pair for the centre
    org + direction*t.  A triangle with a non-finite vertex component has no candidate.  The record is taken as it is: whether it is valid is sphere_sweeps'
    business.  Returns (has[..., n] bool, t[..., n], u[..., n], v[..., n], feature[..., n] int — the index into SWEEP_FEATURES of the first feature at t_tri)."""
    f32 = np.float32
    t_ = np.asarray(tris, dtype=f32)
    verts = t_.reshape(-1, 4, 4)[:, :3, :3] if t_.ndim == 2 and t_.shape[1] == 16 else t_.reshape(-1, 3, 3)
    p, d = np.asarray(org, dtype=f32), np.asarray(direction, dtype=f32)
    single = p.ndim == 1
    p, d = p.reshape(-1, 3), d.reshape(-1, 3)
    r = np.broadcast_to(np.asarray(radius, dtype=f32), p.shape[:1]).astype(f32)
    big_t = np.broadcast_to(np.asarray(tmax, dtype=f32), p.shape[:1]).astype(f32)
    with np.errstate(all="ignore"):
        finite = np.isfinite(verts).all(axis=(1, 2))
        lo, hi = np.fmin(np.fmin(verts[:, 0], verts[:, 1]), verts[:, 2]), np.fmax(np.fmax(verts[:, 0], verts[:, 1]), verts[:, 2])
        passes, t_in = sweep_slab(p[:, None, :], d[:, None, :], r[:, None], big_t[:, None], lo, hi)
        times = sweep_feature_times(p, d, r, big_t, verts)
        t_tri = times.min(axis=-1)
        feature = times.argmin(axis=-1)
        t = np.where(t_in > t_tri, t_in, t_tri)
        has = finite & passes & (t < f32(np.inf))
        t = np.where(has, t, f32(0))
        centre = p[:, None, :] + d[:, None, :] * t[..., None]
        u, v = _closest_point_pairs(centre, verts)[2:4]
    assert t.dtype == f32 and u.dtype == f32
    if single:
        return has[0], t[0], u[0], v[0], feature[0]
    return has, t, u, v, feature


def sweep_records(org, direction, radius, tmax=np.inf) -> np.ndarray:
    """SPHERE_SWEEP_DTYPE[m] with the in quads filled (radius and tmax a scalar or one per record) and the out quad zero."""
    p = np.asarray(org, dtype=np.float32).reshape(-1, 3)
    rec = np.zeros(p.shape[0], dtype=SPHERE_SWEEP_DTYPE)
    rec["org"], rec["dir"] = p, np.asarray(direction, dtype=np.float32).reshape(-1, 3)
    rec["radius"], rec["tmax"] = np.asarray(radius, dtype=np.float32), np.asarray(tmax, dtype=np.float32)
    return rec


def sweep_valid(records) -> np.ndarray:
    """Which records of a SPHERE SWEEP are valid: org and dir finite, radius a finite number >= 0, tmax a number >= 0 (+inf allowed; -0.0 is 0)."""
    rec = np.asarray(records)
    with np.errstate(all="ignore"):
        return np.isfinite(rec["org"]).all(axis=1) & np.isfinite(rec["dir"]).all(axis=1) & np.isfinite(rec["radius"]) & (rec["radius"] >= 0) & (rec["tmax"] >= 0)


def sphere_sweeps(tris, records, perm=None, chunk: int = 1 << 18, features=None) -> np.ndarray:
    """The normative statement of a SPHERE SWEEP (include/rvpt_hip.h: SPHERE SWEEPS), by brute force: every triangle's candidate (t_i, prim_i) from
    sweep_sphere_triangles, the answer the lexicographically smallest one — among equal t the smaller reported number, which is the index, or perm[index] with
    a permutation.  `tris` (float32[n, 16]) in stored order; `records` SPHERE_SWEEP_DTYPE[m].  An invalid record (sweep_valid) and a miss go out as t = the bits
    of tmax, prim NO_PRIM, u = v = 0.  Returns a copy of `records` with the out quads written and the in quads as they came.  `features`, an int array [m], is
    filled with the deciding feature of each hit (the index into SWEEP_FEATURES) and -1 elsewhere."""
    rec = np.asarray(records)
    if rec.dtype != SPHERE_SWEEP_DTYPE:
        raise ValueError(f"sphere_sweeps: SPHERE_SWEEP_DTYPE records are needed, got {rec.dtype}")
    out = np.ascontiguousarray(rec).copy().reshape(-1)
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    n = t.shape[0]
    number = np.arange(n, dtype=np.uint32) if perm is None else np.asarray(perm, dtype=np.uint32).reshape(n)
    out["t"], out["prim"], out["u"], out["v"] = out["tmax"], NO_PRIM, 0, 0
    if features is not None:
        features[...] = -1
    rows = np.flatnonzero(sweep_valid(out))
    step = max(1, chunk // max(n, 1))
    for at in range(0, rows.size if n else 0, step):
        sel = rows[at:at + step]
        has, tt, u, v, feature = sweep_sphere_triangles(out["org"][sel], out["dir"][sel], out["radius"][sel], out["tmax"][sel], t)
        key = np.where(has, tt, np.float32(np.inf))
        best = has & (key == key.min(axis=1, keepdims=True))
        hit = best.any(axis=1)
        i = np.argmin(np.where(best, number[None, :].astype(np.int64), np.int64(1) << 40), axis=1)  # the smallest reported number among equal t
        k = np.arange(sel.size)
        got = out[sel]
        got["t"][hit], got["prim"][hit], got["u"][hit], got["v"][hit] = tt[k, i][hit], number[i][hit], u[k, i][hit], v[k, i][hit]
        out[sel] = got
        if features is not None:
            features[sel] = np.where(hit, feature[k, i], -1)
    return out.reshape(rec.shape)


SURFACE_POINT_DTYPE =np.dtype([("prim", "<u4"), ("u", "<f4"), ("v", "<f4"), ("flags", "<u4"), ("point", "<f4", (3,)), ("mat", "<u4"), ("normal", "<f4", (3,)),
                                ("reserved", "<u4")])  # rvpt_surface_point (== native.SURFACE_POINT_DTYPE)
_LIBM_FMAF = None


def _fmaf(x, y, z) -> np.ndarray:
    """fma(x, y, z) in float32 with ONE rounding, element by element through libm's fmaf (Python 3.10 has no math.fma, and numpy never fuses)."""
    global _LIBM_FMAF
    if _LIBM_FMAF is None:
        import ctypes
        import ctypes.util
        libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        libm.fmaf.restype = ctypes.c_float
        libm.fmaf.argtypes = [ctypes.c_float] * 3
        _LIBM_FMAF = libm.fmaf
    x, y, z = np.broadcast_arrays(np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32), np.asarray(z, dtype=np.float32))
    out = np.empty(x.shape, dtype=np.float32)
    flat = out.reshape(-1)
    for k, (a, b, c) in enumerate(zip(x.reshape(-1).tolist(), y.reshape(-1).tolist(), z.reshape(-1).tolist())):
        flat[k] = _LIBM_FMAF(a, b, c)
    return out


def triangle_unit_normals(tris) -> np.ndarray:
    """The hit normal the library stores per triangle (rvpt_kernels.hip: prepare_triangles; intersection.glsl:511-513), float32[n, 3]:
    normalize(cross(vert1 - vert0, vert2 - vert0)) by rvpt_math.h — cross with every product and difference rounded on its own, the squared length by the FUSED
    dot fma(z, z, fma(y, y, x*x)), its square root and the quotient 1 / len correctly rounded, then one product per component.  Not turned towards any ray.  A
    zero-area triangle gets what this arithmetic gives (0 * inf = NaN)."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    a, b, c = t[:, 0:3], t[:, 4:7], t[:, 8:11]
    with np.errstate(all="ignore"):
        e0, e1 = b - a, c - a
        nn = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1], e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2], e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]], axis=1)
        sq = _fmaf(nn[:, 2], nn[:, 2], _fmaf(nn[:, 1], nn[:, 1], nn[:, 0] * nn[:, 0]))
        inv = np.float32(1) / np.sqrt(sq)
        out = nn * inv[:, None]
    assert out.dtype == np.float32
    return out


def surface_points(tris, prim, u, v) -> np.ndarray:
    """The normative statement of a SURFACE POINT read (include/rvpt_hip.h: SURFACE POINTS).  `tris` (float32[n, 16]) in the order the update form takes on the
    context asked, which is the numbering of prim.  Per record, with a, b, c = vert0..2 of triangle prim: point = (a + (b-a)*u) + (c-a)*v per component in
    float32, every operation rounded on its own (numpy never fuses) — u weights vert1 - vert0, v weights vert2 - vert0, any finite pair is evaluated; normal =
    triangle_unit_normals of the row; mat = int(mat_id.x) as a uint32 word.  prim >= n or a non-finite u or v: point = normal = 0, mat = 0xFFFFFFFF.  reserved is 0.
    Returns SURFACE_POINT_DTYPE[m] with the in fields filled (flags 0)."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    prim = np.asarray(prim, dtype=np.uint32).reshape(-1)
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    rec = np.zeros(prim.shape[0], dtype=SURFACE_POINT_DTYPE)
    rec["prim"], rec["u"], rec["v"] = prim, u, v
    rec["mat"] = NO_PRIM
    valid = (prim < t.shape[0]) & np.isfinite(rec["u"]) & np.isfinite(rec["v"])
    rows = np.flatnonzero(valid)
    if rows.size == 0:
        return rec
    used, where = np.unique(prim[rows], return_inverse=True)
    normals = triangle_unit_normals(t[used])[where]
    tri = t[prim[rows]]
    a, b, c = tri[:, 0:3], tri[:, 4:7], tri[:, 8:11]
    uu, vv = rec["u"][rows][:, None], rec["v"][rows][:, None]
    with np.errstate(all="ignore"):
        point = (a + (b - a) * uu) + (c - a) * vv
        mat = tri[:, 12].astype(np.int32).astype(np.uint32)
    assert point.dtype == np.float32
    out = rec[rows]
    out["point"], out["normal"], out["mat"] = point, normals, mat
    rec[rows] = out
    return rec


def load_obj_positions(path) -> np.ndarray:
    """Minimal Wavefront OBJ reader: `v` records and `f` records (v, v/vt, v/vt/vn, v//vn, negative
    indices); polygons are fan-triangulated (tinyobjloader's default `triangulate=true`, which is
    what main.cpp:23 uses); normals/uvs/materials are ignored like load_model() (main.cpp:49-59).
    Returns float32[n_tris,3,3]."""
    verts: list[tuple[float, float, float]] = []
    faces: list[tuple[int, int, int]] = []
    with open(path, "r") as f:
        for line in f:
            if line.startswith("v "):
                a = line.split()
                verts.append((float(a[1]), float(a[2]), float(a[3])))
            elif line.startswith("f "):
                idx = []
                for tok in line.split()[1:]:
                    i = int(tok.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[k], idx[k + 1]))
    v = np.asarray(verts, dtype=np.float32)
    fi = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return v[fi]


def load_mtl(path) -> dict:
    """Wavefront MTL -> {name: material[12]} in the reference Material layout (material.h:9-26).

    The reference's loader ignores materials (main.cpp:49-59: constant material id); this is the scene-description
    step SURVEY §8(f-2) asks for.  Mapping: `Kd` -> albedo, `Ke` -> emission, `Ni` -> index of refraction
    (albedo.w, intersection.glsl:54); type from `illum`: 3 / 8 (reflection without refraction) -> MIRROR with
    albedo `Ks` when given, 4 / 6 / 7 / 9 (glass / refraction) or `d` < 1 -> DIELECTRIC, anything else -> LAMBERT."""
    mats: dict = {}
    cur = None
    with open(path, "r") as f:
        for line in f:
            a = line.split()
            if not a or a[0].startswith("#"):
                continue
            if a[0] == "newmtl":
                cur = {"Kd": (0.8, 0.8, 0.8), "Ke": (0.0, 0.0, 0.0), "Ks": None, "Ni": 1.5, "illum": 2, "d": 1.0}
                mats[" ".join(a[1:])] = cur
            elif cur is None:
                continue
            elif a[0] in ("Kd", "Ke", "Ks") and len(a) >= 4:
                cur[a[0]] = (float(a[1]), float(a[2]), float(a[3]))
            elif a[0] == "Ni":
                cur["Ni"] = float(a[1])
            elif a[0] == "illum":
                cur["illum"] = int(float(a[1]))
            elif a[0] == "d":
                cur["d"] = float(a[1])
            elif a[0] == "Tr":
                cur["d"] = 1.0 - float(a[1])
    out = {}
    for name, m in mats.items():
        if m["illum"] in (3, 8):
            out[name] = make_material((*(m["Ks"] or m["Kd"]), 0.0), (*m["Ke"], 0.0), MIRROR)
        elif m["illum"] in (4, 6, 7, 9) or m["d"] < 1.0:
            out[name] = make_material((*m["Kd"], m["Ni"]), (*m["Ke"], 0.0), DIELECTRIC)
        else:
            out[name] = make_material((*m["Kd"], 0.0), (*m["Ke"], 0.0), LAMBERT)
    return out


def load_obj_scene(path):
    """OBJ + MTL -> (tris[n,16], mats[m,12], names[m]): `mtllib` files are read relative to the OBJ, `usemtl`
    selects the material of the faces that follow.  Material ids are handed out in order of first use; faces
    before any `usemtl`, or naming a material no library defines, get a white Lambert material called "default"."""
    import os
    verts: list[tuple[float, float, float]] = []
    faces: list[tuple[int, int, int]] = []
    face_mat: list[int] = []
    library: dict = {}
    names: list[str] = []
    mats: list[np.ndarray] = []
    ids: dict = {}

    def material_id(name):
        key = name if name in library else "default"
        if key not in ids:
            ids[key] = len(names)
            names.append(key)
            mats.append(library[key] if key in library else make_material((1, 1, 1, 0), (0, 0, 0, 0), LAMBERT))
        return ids[key]

    cur = None
    base = os.path.dirname(os.path.abspath(path))
    with open(path, "r") as f:
        for line in f:
            a = line.split()
            if not a:
                continue
            if a[0] == "v":
                verts.append((float(a[1]), float(a[2]), float(a[3])))
            elif a[0] == "mtllib":
                for lib in a[1:]:
                    lp = os.path.join(base, lib)
                    if os.path.exists(lp):
                        library.update(load_mtl(lp))
            elif a[0] == "usemtl":
                cur = " ".join(a[1:])
            elif a[0] == "f":
                idx = []
                for tok in a[1:]:
                    i = int(tok.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                mid = material_id(cur if cur is not None else "default")
                for k in range(1, len(idx) - 1):
                    faces.append((idx[0], idx[k], idx[k + 1]))
                    face_mat.append(mid)
    v = np.asarray(verts, dtype=np.float32)
    fi = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    tris = make_triangles(v[fi], 0)
    tris[:, 12] = np.asarray(face_mat, dtype=np.float32)
    return tris, np.stack(mats) if mats else np.zeros((0, 12), np.float32), names


def write_obj(path, positions) -> None:
    """Write de-indexed triangles as OBJ text (used to route generated scenes through the OBJ path)."""
    p = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    with open(path, "w") as f:
        f.write("# generated by rvpt_amd.scene.write_obj\n")
        for x, y, z in p:
            f.write(f"v {float(x):.9g} {float(y):.9g} {float(z):.9g}\n")
        for t in range(p.shape[0] // 3):
            f.write(f"f {3*t+1} {3*t+2} {3*t+3}\n")


def write_obj_scene(path, tris, mats) -> None:
    """Write (tris[n,16], mats[m,12]) as OBJ + MTL (same stem) so that load_obj_scene() / load_scene() read back the
    same triangles with the same material per triangle (ids are renumbered in order of first use)."""
    import os
    tris = np.asarray(tris, dtype=np.float32).reshape(-1, 16)
    mats = np.asarray(mats, dtype=np.float32).reshape(-1, 12)
    stem = os.path.splitext(str(path))[0]
    with open(stem + ".mtl", "w") as f:
        f.write("# generated by rvpt_amd.scene.write_obj_scene\n")
        for i, m in enumerate(mats):
            t = int(m[8])
            f.write(f"newmtl m{i}\n")
            f.write("Kd {:.9g} {:.9g} {:.9g}\n".format(*map(float, m[0:3])))
            f.write("Ke {:.9g} {:.9g} {:.9g}\n".format(*map(float, m[4:7])))
            if t == MIRROR:
                f.write("Ks {:.9g} {:.9g} {:.9g}\nillum 3\n".format(*map(float, m[0:3])))
            elif t == DIELECTRIC:
                f.write(f"Ni {float(m[3]):.9g}\nillum 7\n")
            else:
                f.write("illum 2\n")
    ids = tris[:, 12].astype(np.int64)
    with open(path, "w") as f:
        f.write("# generated by rvpt_amd.scene.write_obj_scene\n")
        f.write(f"mtllib {os.path.basename(stem)}.mtl\n")
        for t in tris:
            for k in (0, 4, 8):
                f.write(f"v {float(t[k]):.9g} {float(t[k+1]):.9g} {float(t[k+2]):.9g}\n")
        cur = None
        for i in range(tris.shape[0]):
            if ids[i] != cur:
                cur = ids[i]
                f.write(f"usemtl m{cur}\n")
            f.write(f"f {3*i+1} {3*i+2} {3*i+3}\n")


def default_model_positions() -> np.ndarray:
    """De-indexed positions of the default model (143 triangles), see tools/make_default_scene.py."""
    return np.fromfile(_ASSETS / "default_scene_tris.f32", dtype="<f4").reshape(-1, 3, 3).copy()


def default_materials() -> np.ndarray:
    """main.cpp:105-107: id 0 emissive Lambert (unused by the model), id 1 white Lambert."""
    return np.stack([
        make_material((1, 1, 1, 0), (0.1, 0.4, 0.6, 0), LAMBERT),
        make_material((1, 1, 1, 0), (0, 0, 0, 0), LAMBERT),
    ])


def default_scene():
    """(tris[143,16], mats[2,12]) exactly as main() builds them (main.cpp:102-107)."""
    return make_triangles(default_model_positions(), 1), default_materials()


def subdivide(positions, levels: int) -> np.ndarray:
    """Midpoint 1->4 subdivision, `levels` times (deterministic)."""
    p = np.asarray(positions, dtype=np.float32).reshape(-1, 3, 3)
    for _ in range(levels):
        a, b, c = p[:, 0], p[:, 1], p[:, 2]
        ab, bc, ca = ((a + b) * np.float32(0.5)), ((b + c) * np.float32(0.5)), ((c + a) * np.float32(0.5))
        p = np.concatenate([
            np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)
        ]).astype(np.float32)
    return p


def _quad(p0, p1, p2, p3):
    return np.array([[p0, p1, p2], [p0, p2, p3]], dtype=np.float32)


def cornell_scene(subdiv_levels: int = 3):
    """BASELINE config 3: Cornell box (5 walls + ceiling light = 12 triangles) around the default model
    subdivided `subdiv_levels` times (143*4^3 = 9152 triangles).  Materials: 0 white .73, 1 red,
    2 green, 3 light (emission 15), 4 model (Lambert .8).  Box spans x,z in [-2,2], y in [0,4]."""
    lo, hi, y0, y1 = -2.0, 2.0, 0.0, 4.0
    parts, mat_ids = [], []

    def add(q, m):
        parts.append(q)
        mat_ids.extend([m] * q.shape[0])

    add(_quad((lo, y0, lo), (hi, y0, lo), (hi, y0, hi), (lo, y0, hi)), 0)  # floor
    add(_quad((lo, y1, lo), (lo, y1, hi), (hi, y1, hi), (hi, y1, lo)), 0)  # ceiling
    add(_quad((lo, y0, hi), (hi, y0, hi), (hi, y1, hi), (lo, y1, hi)), 0)  # back wall (z = hi)
    add(_quad((lo, y0, lo), (lo, y0, hi), (lo, y1, hi), (lo, y1, lo)), 1)  # left, red
    add(_quad((hi, y0, lo), (hi, y1, lo), (hi, y1, hi), (hi, y0, hi)), 2)  # right, green
    add(_quad((-0.6, y1 - 0.01, -0.6), (-0.6, y1 - 0.01, 0.6), (0.6, y1 - 0.01, 0.6), (0.6, y1 - 0.01, -0.6)), 3)
    model = subdivide(default_model_positions(), subdiv_levels)
    add(model, 4)
    pos = np.concatenate(parts)
    ids = np.asarray(mat_ids)
    tris = make_triangles(pos, 0)
    tris[:, 12] = ids.astype(np.float32)
    mats = np.stack([
        make_material((0.73, 0.73, 0.73, 0), (0, 0, 0, 0), LAMBERT),
        make_material((0.65, 0.05, 0.05, 0), (0, 0, 0, 0), LAMBERT),
        make_material((0.12, 0.45, 0.15, 0), (0, 0, 0, 0), LAMBERT),
        make_material((0.0, 0.0, 0.0, 0), (15, 15, 15, 0), LAMBERT),
        make_material((0.8, 0.8, 0.8, 0), (0, 0, 0, 0), LAMBERT),
    ])
    return tris, mats


def _value_noise(n: int, seed: int, octaves: int = 3) -> np.ndarray:
    rng = np.random.RandomState(seed)
    h = np.zeros((n, n), dtype=np.float64)
    xs = np.linspace(0.0, 1.0, n)
    amp, cells = 1.0, 4
    for _ in range(octaves):
        g = rng.rand(cells + 2, cells + 2)
        fx = xs * cells
        i = np.minimum(fx.astype(np.int64), cells - 1)
        t = fx - i
        t = t * t * (3 - 2 * t)
        rows = g[i][:, i] * (1 - t)[None, :] + g[i][:, i + 1] * t[None, :]
        rows1 = g[i + 1][:, i] * (1 - t)[None, :] + g[i + 1][:, i + 1] * t[None, :]
        h += amp * (rows * (1 - t)[:, None] + rows1 * t[:, None])
        amp *= 0.5
        cells *= 2
    return h


def heightfield_scene(cells: int = 708, seed: int = 1234):
    """BASELINE config 4: cells x cells grid, 2 triangles per cell (708 -> 1 002 528 triangles), height =
    3-octave value noise.  Spans x,z in [-4,4], y in [0,~1.2]; material 0 = Lambert .7 grey."""
    n = cells + 1
    h = (_value_noise(n, seed) * 0.7).astype(np.float32)
    xs = np.linspace(-4.0, 4.0, n, dtype=np.float32)
    X, Z = np.meshgrid(xs, xs, indexing="xy")
    P = np.stack([X, h, Z], axis=-1)  # [n,n,3], P[j,i] = (x_i, h, z_j)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t0 = np.stack([p00, p01, p11], axis=2).reshape(-1, 3, 3)
    t1 = np.stack([p00, p11, p10], axis=2).reshape(-1, 3, 3)
    pos = np.concatenate([t0, t1]).astype(np.float32)
    mats = np.stack([make_material((0.7, 0.7, 0.7, 0), (0, 0, 0, 0), LAMBERT)])
    return make_triangles(pos, 0), mats


def materials_showcase_scene():
    """Small scene exercising all three material types + an emitter (parity stress for the
    mirror / dielectric branches of integrator_Kajiya, integrators.glsl:625-665)."""
    model = default_model_positions()
    parts = [model]
    ids = [2] * model.shape[0]  # glass model
    fl = _quad((-3, 0.0, -3), (3, 0.0, -3), (3, 0.0, 3), (-3, 0.0, 3))
    parts.append(fl); ids += [0, 0]
    mir = _quad((-3, 0.0, 2.0), (3, 0.0, 2.0), (3, 3.0, 2.0), (-3, 3.0, 2.0))
    parts.append(mir); ids += [1, 1]
    light = _quad((-1, 3.5, -1), (-1, 3.5, 1), (1, 3.5, 1), (1, 3.5, -1))
    parts.append(light); ids += [3, 3]
    tris = make_triangles(np.concatenate(parts), 0)
    tris[:, 12] = np.asarray(ids, dtype=np.float32)
    mats = np.stack([
        make_material((0.6, 0.6, 0.6, 0), (0, 0, 0, 0), LAMBERT),
        make_material((0.9, 0.9, 0.9, 0), (0, 0, 0, 0), MIRROR),
        make_material((0.95, 0.95, 0.95, 1.5), (0, 0, 0, 0), DIELECTRIC),
        make_material((0, 0, 0, 0), (8, 8, 8, 0), LAMBERT),
    ])
    return tris, mats
