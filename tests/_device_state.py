"""Host statements of what a BVH context holds on the device, in numpy, for tests/test_device_state.py: the inputs, upload_scene's breadth-first relayout with its
level table, the head-shift rule, the expected 4-wide form and the sparse update's maps.  A plain module: no fixture, no GPU."""
import numpy as np

from rvpt_amd import native, scene

NODE = native.NODE_DTYPE
EMPTY = 0xFFFFFFFF


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------------------

def _records(p, rng):
    """positions float32[n, 3, 3] -> float32[n, 16] with a random material row: a valid index into default_materials() and three words nothing reads"""
    t = scene.make_triangles(p, 0)
    t[:, 12] = rng.randint(0, scene.default_materials().shape[0], t.shape[0]).astype(np.float32)
    t[:, 13:16] = rng.uniform(-9.0, 9.0, (t.shape[0], 3)).astype(np.float32)
    return t


def soup(n, seed):
    """uniform random centres in [-4, 4]^3, vertex offsets in +-0.3"""
    rng = np.random.RandomState(seed)
    p = (rng.uniform(-4.0, 4.0, (n, 1, 3)) + rng.uniform(-0.3, 0.3, (n, 3, 3))).astype(np.float32)
    return _records(p, rng)


def lattice(n, seed):
    """centres rounded to integers, offsets to halves, the whole shifted by +0.25 (the unshifted lattice holds -0): many equal centroids, equal Morton codes, equal
    PLOC distances and, for the SAH build, median splits"""
    rng = np.random.RandomState(seed)
    c, o = np.round(rng.uniform(-4.0, 4.0, (n, 1, 3))), np.round(rng.uniform(-0.3, 0.3, (n, 3, 3)) * 2.0) / 2.0
    return _records((c + o + 0.25).astype(np.float32), rng)


SOUPS = {"soup": soup, "lattice": lattice}


def ladder(rungs, cluster, seed, top=2.0 ** 75, ratio=1.0 / 32.0, h=2.0 ** -60):
    """A geometric ladder along x: `rungs` triangles at top * ratio^k, then `cluster` triangles within [1/4, 1) of top * ratio^rungs; each is (x, h, h)
    (x + x/64, 2h, h) (x, h, 2h), the rows shuffled.  Centroid y and z are one float32 for all, so only axis 0 is live; a rung lies more than 16 times further
    out than everything below it, so it falls alone into bin 15 and the rest into bin 0: the SAH build peels one triangle per level and meets the cluster at
    depth `rungs` — 30 is rv::kSahBalanceDepth, from where on only median splits are made.  h is below the smallest extent in x, every box area is a normal
    float32 (about 2^16 down to 2^-115), no coordinate is zero.  NOT one of SOUPS: a few tests name it, the parametrised ones do not take it."""
    rng = np.random.RandomState(seed)
    xs = np.concatenate([top * ratio ** np.arange(rungs), top * ratio ** rungs * rng.uniform(0.25, 1.0, cluster)])  # float64
    p = np.empty((xs.shape[0], 3, 3), dtype=np.float64)
    p[:, 0] = np.stack([xs, np.full_like(xs, h), np.full_like(xs, h)], axis=1)
    p[:, 1] = np.stack([xs + xs / 64.0, np.full_like(xs, 2.0 * h), np.full_like(xs, h)], axis=1)
    p[:, 2] = np.stack([xs, np.full_like(xs, h), np.full_like(xs, 2.0 * h)], axis=1)
    t = scene.make_triangles(p.astype(np.float32), 0)
    return np.ascontiguousarray(t[rng.permutation(t.shape[0])])


# the ladders the tests build: (rungs, cluster, seed) -> what scene.build_sah reports; the rows are, in order: the plain case; a node of 5000 > kSahLargeNode at depth 30
# and two of 2500 at depth 31, large nodes whose bin launch is skipped; the cluster's first split at depth 29, still binned; nine triangles at depth 30 (one
# median split); eight (a leaf: no median split at all)
LADDERS = {
    (30, 300, 1): {"n": 330, "height": 37, "binned_splits": 30, "median_splits": 63, "max_leaf": 5},
    (30, 5000, 2): {"n": 5030, "height": 41, "binned_splits": 30, "median_splits": 1023, "max_leaf": 5},
    (29, 300, 3): {"n": 329, "height": 36, "binned_splits": 30, "median_splits": 62, "max_leaf": 5},
    (30, 9, 4): {"n": 39, "height": 32, "binned_splits": 30, "median_splits": 1, "max_leaf": 5},
    (30, 8, 5): {"n": 38, "height": 31, "binned_splits": 30, "median_splits": 0, "max_leaf": 8},
}
# The first row squeezed into the binades in which a ray can hit its cluster (tests/test_ray_query.py).  The reference's triangle test divides by
# det = |e0|^2 |e1|^2 - (e0 . e1)^2 = (dx^2 + h^2) h^2 with dx = x / 64: with the defaults above that is 2^-240 for every triangle of the cluster, zero in float32,
# and no ray whatever hits one.  Here a rung lies 17 times further out than the next (still alone in bin 15), dx >= 2^-30 and h = 2^-32: det >= 2^-124, a normal float32.  The
# eight rungs furthest out (dx >= 2^66, dx^2 = inf) stay beyond any ray.  scene.build_sah reports what it reports for the first row.
HITTABLE_LADDER = {"rungs": 30, "cluster": 300, "seed": 1, "top": 2.0 ** 101, "ratio": 1.0 / 17.0, "h": 2.0 ** -32}


def vertices(tris):
    """the nine coordinates of every triangle, float32[n, 3, 3] (a view where `tris` is contiguous)"""
    return np.asarray(tris).reshape(-1, 4, 4)[:, :3, :3]


def no_zero_coordinate(tris) -> bool:
    """the condition under which min / max, hence byte equality of boxes, is well defined: no vertex coordinate is +-0 (NaN and infinities are not zeros)"""
    return not bool((vertices(tris) == 0).any())


def with_non_finite(tris, seed, whole_axis=None):
    """about 2 % of the triangles get NaN, +inf or -inf: half of them in ONE coordinate, half in all nine; whole_axis: every triangle's coordinates on that
    axis are NaN as well.  Returns (triangles, the indices changed)."""
    rng = np.random.RandomState(seed)
    t = np.array(tris, dtype=np.float32)
    n = t.shape[0]
    k = max(3, n // 50)
    pick = rng.permutation(n)[:k]
    values = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    v = vertices(t)
    for j, i in enumerate(pick):
        val = values[j % 3]
        if (j // 3) % 2 == 0:
            v[i, rng.randint(3), rng.randint(3)] = val
        else:
            v[i] = val
    if whole_axis is not None:
        v[:, :, whole_axis] = np.nan
    return t, np.sort(pick)


def shrunk(tris, idx, factor=0.5):
    """the triangles `idx` scaled towards their own centroids"""
    t = np.array(tris, dtype=np.float32)
    v = vertices(t)
    c = v[idx].astype(np.float64).mean(axis=1, keepdims=True)
    v[idx] = (c + factor * (v[idx].astype(np.float64) - c)).astype(np.float32)
    return t


# ---- the device layout --------------------------------------------------------------------------------------------------------------------------------------

def device_layout(nodes):
    """upload_scene's relayout (rvpt_scene.hip): a FIFO from the root — root at 0, slot 1 zero, the children of every inner node taken from the queue at the next
    free pair 2, 4, ..; nodes the root does not reach never arrive.  Returns (NODE records [len(nodes) + 1], levels uint32[h, 2] = [begin, end) per level)."""
    src = np.ascontiguousarray(nodes).view(NODE).reshape(-1)
    first, count = src["first"].tolist(), src["count"].tolist()
    queue_src, queue_dst, new_first, levels = [0], [0], [], []
    next_pair, level_end, head = 2, 0, 0
    while head < len(queue_src):
        if head == level_end:
            levels.append((queue_dst[head], queue_dst[-1] + 1))
            level_end = len(queue_src)
        s = queue_src[head]
        head += 1
        if count[s] == 0:
            new_first.append(next_pair)
            queue_src += [first[s], first[s] + 1]
            queue_dst += [next_pair, next_pair + 1]
            next_pair += 2
        else:
            new_first.append(first[s])
    out = np.zeros(src.shape[0] + 1, dtype=NODE)
    out[queue_dst] = src[queue_src]
    out["first"][queue_dst] = new_first
    return out, np.array(levels, dtype=np.uint32).reshape(-1, 2)


def shifted_layout(nodes):
    """the same for a tree that is already breadth first (every numpy builder's): every index after the root plus one.  tests/test_device_state.py asserts the
    identity with device_layout on the CPU."""
    src = np.ascontiguousarray(nodes).view(NODE).reshape(-1)
    out = np.zeros(src.shape[0] + 1, dtype=NODE)
    out[0] = src[0]
    out[2:] = src[1:]
    inner = out["count"] == 0
    inner[1] = False
    out["first"][inner] += 1
    return out


def levels_of(dev_nodes):
    """the level table of a tree in the device layout: a level's nodes are contiguous, the next level starts at the first child of its first inner node"""
    first, count = dev_nodes["first"].astype(np.int64), dev_nodes["count"].astype(np.int64)
    levels, begin, end = [], 0, 1
    while True:
        levels.append((begin, end))
        inner = np.flatnonzero(count[begin:end] == 0) + begin
        if inner.size == 0:
            break
        assert np.array_equal(first[inner], first[inner[0]] + 2 * np.arange(inner.size)), "not a breadth-first layout"
        begin, end = int(first[inner[0]]), int(first[inner[0]]) + 2 * inner.size
    return np.array(levels, dtype=np.uint32).reshape(-1, 2)


def head_shift(n_device_nodes, n_tris, max_count):
    """rvpt_scene.hip's rule: indices of the device layout and of the triangles below 2^shift, leaf sizes below 2^(32 - shift); 0: heads do not pack"""
    shift = 1
    while shift < 31 and (1 << shift) <= max(n_device_nodes, n_tris):
        shift += 1
    return shift if max_count < (1 << (32 - shift)) else 0


class Expected:
    """everything a context holds after upload_scene(nodes, tris, mats) / a build form whose numpy statement returned `nodes`"""

    def __init__(self, nodes, breadth_first=False):
        """breadth_first: `nodes` come from a numpy builder, whose layout is breadth first already (shifted_layout, much the quicker for 80 000 nodes)"""
        self.nodes, self.levels = (shifted_layout(nodes), None) if breadth_first else device_layout(nodes)
        if self.levels is None:
            self.levels = levels_of(self.nodes)
        rec = self.nodes
        self.n_nodes = rec.shape[0]
        self.height = self.levels.shape[0]
        live = np.ones(self.n_nodes, dtype=bool)
        live[1] = False
        leaves = live & (rec["count"] > 0)
        self.n_tris = int((rec["first"][leaves].astype(np.int64) + rec["count"][leaves]).max())
        self.head_shift = head_shift(self.n_nodes, self.n_tris, int(rec["count"].max()))
        wide, need = native.wide_form(rec, self.head_shift)
        keep = wide.shape[0] > 0 and need <= 4096
        self.wide = wide if keep else wide[:0]
        self.wide_stack_levels = need if keep else 0
        # the sparse update's maps
        self.parent = np.full(self.n_nodes, EMPTY, dtype=np.uint32)
        inner = np.flatnonzero(live & (rec["count"] == 0))
        self.parent[rec["first"][inner]] = inner
        self.parent[rec["first"][inner] + 1] = inner
        self.leaf_of = np.full(self.n_tris, EMPTY, dtype=np.uint32)
        for i in np.flatnonzero(leaves):
            self.leaf_of[rec["first"][i]: rec["first"][i] + rec["count"][i]] = i
        self.n_map_nodes = int(self.levels[-1, 1])  # the maps end with the last level (a root leaf: one word, the layout has two slots)


def regathered(wide, wide_map, dev_nodes):
    """refit_wide_gather in numpy: every used slot takes the six bounds of its binary node; heads and padding stay"""
    out = wide.copy()
    w, s = np.nonzero(wide_map != EMPTY)
    b = dev_nodes["bounds"][wide_map[w, s]]
    for q in range(6):
        out[w, q, s] = b[:, q]
    return out


def check_wide_map(state, what=""):
    """d_wide_map against d_nodes and d_wide: slot s of wide node w names a binary node whose six bounds are the bytes in that slot; unused slots are 0xFFFFFFFF in
    both map and head; a leaf slot's head is its leaf's first | count << shift; and the structure — wide node 0 stands for the root, the wide node an inner
    slot's head names stands for that slot's binary node, and the used slots of a wide node are, in order, what its binary node's child list [left, right]
    becomes when inner entries are replaced in place by their two children (rvpt_bvh_wide_form's regrouping): that pins every word of the map."""
    wide, wmap, nodes = state["wide"], state["wide_map"], state["nodes"]
    assert wmap.shape == (wide.shape[0], 4), what
    if wide.shape[0] == 0:
        return
    heads = wide[:, 6, :].view(np.uint32)
    unused = wmap == EMPTY
    assert np.array_equal(unused, heads == EMPTY), what
    w, s = np.nonzero(~unused)
    assert (wmap[w, s] < nodes.shape[0]).all() and (wmap[w, s] != 1).all(), what
    got = np.stack([wide[w, q, s] for q in range(6)], axis=1)
    assert got.view(np.uint32).tobytes() == np.ascontiguousarray(nodes["bounds"][wmap[w, s]]).view(np.uint32).tobytes(), what
    shift = int(state["bvh_head_shift"])
    rec = nodes[wmap[w, s]]
    leaf = rec["count"] > 0
    assert np.array_equal(heads[w, s][leaf], rec["first"][leaf] | (rec["count"][leaf] << np.uint32(shift))), what
    assert (heads[w, s][~leaf] < wide.shape[0]).all(), what
    first, count = nodes["first"].astype(np.int64), nodes["count"].astype(np.int64)
    binary_of = np.full(wide.shape[0], -1, dtype=np.int64)
    binary_of[0] = 0
    for wi in range(wide.shape[0]):  # breadth first: the slot that names a wide node comes before it
        b = int(binary_of[wi])
        assert b >= 0 and count[b] == 0, f"{what}: wide node {wi} stands for no inner binary node"
        slots = [int(x) for x in wmap[wi] if x != EMPTY]
        assert [int(x) for x in wmap[wi][:len(slots)]] == slots and len(slots) >= 2, f"{what}: wide node {wi} has a gap in its slots"
        pos, stack = 0, [int(first[b]) + 1, int(first[b])]
        while stack:  # the child list, left to right: an entry is the next slot, or an inner node whose two children stand in its place
            node = stack.pop()
            if pos < len(slots) and node == slots[pos]:
                pos += 1
            else:
                assert count[node] == 0 and len(stack) < 4, f"{what}: the slots {slots} of wide node {wi} are no expansion of binary node {b}"
                stack += [int(first[node]) + 1, int(first[node])]
        assert pos == len(slots), f"{what}: the slots {slots} of wide node {wi} are no expansion of binary node {b}"
        for si, node in enumerate(slots):
            if count[node] == 0:
                child = int(heads[wi, si])
                assert binary_of[child] == -1, f"{what}: wide node {child} is named twice"
                binary_of[child] = node
    assert (binary_of >= 0).all(), what


# ---- comparisons --------------------------------------------------------------------------------------------------------------------------------------------

def same_bytes(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_floats_nan_in_place(a, b) -> bool:
    """the one comparison of floats that is not of bytes (non-finite inputs only): NaN in the same places, every other word equal bit for bit"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def same_nodes(got, want, nan_in_place=False) -> bool:
    got, want = np.ascontiguousarray(got).view(NODE).reshape(-1), np.ascontiguousarray(want).view(NODE).reshape(-1)
    if not nan_in_place:
        return same_bytes(got, want)
    return got.shape == want.shape and np.array_equal(got["first"], want["first"]) and np.array_equal(got["count"], want["count"]) and \
        same_floats_nan_in_place(got["bounds"], want["bounds"])


def first_difference(got, want):
    """for a failure message: (index, got, want) of the first record that differs"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return ("shape", got.shape, want.shape)
    g, w = got.reshape(got.shape[0], -1).view(np.uint8), want.reshape(want.shape[0], -1).view(np.uint8)
    bad = np.flatnonzero((g != w).any(axis=1))
    return None if bad.size == 0 else (int(bad[0]), got[bad[0]], want[bad[0]], f"{bad.size} records differ")
