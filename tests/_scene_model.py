"""The numpy statement of what ONE context holds of its geometry across every form of rvpt_hip_upload_scene (include/rvpt_hip.h), and a seeded generator of
steps that walks those forms in random order, for tests/test_scene_model_host.py, tests/test_update_sequences.py and tools/fuzz_updates.py.

`Model` has one method per form; each applies the header's rule and nothing else, and is built only from the statements the forms already have:
scene.refit_bvh(..., touched=), scene.tree_cost, scene.pose_parts, scene.skin_triangles, scene.build_lbvh / build_ploc / build_sah and the layout helpers of
tests/_device_state.py.  A method returns what the call reports — None, or (cost, base, rebuilt, tree name, new base) — and where the header refuses it raises
Refused(pattern) and leaves the model as it was.  Methods never write into an array the model holds: they replace it, so a shallow copy is a snapshot.

Everything is in the order the plain update form takes (the caller's order after a build form, the leaf order after an ordinary upload) except what `perm`
is applied to.  A plain module: no fixture, no GPU."""
import copy
import math
from typing import NamedTuple, Optional

import numpy as np

import _device_state as ds
import _guarded_pose as gp
import _guarded_skin as gs
import _skin
from rvpt_amd import native, scene

EMPTY = ds.EMPTY
BUILDERS = ("lbvh", "ploc", "sah")
SOURCES = ("upload", "upload-loose", "lbvh", "ploc", "sah", "brute")
MAX_TRIS = 640
MAX_STEPS = 32
MAX_SEQUENCES = 24
REDRAWS = 8
MARGIN = 1e-6  # the least distance of cost / (limit x base) from 1 a guarded step may have: a thousand times test_guarded_update.REL

# the thirteen successful forms whose ordered pairs the walk covers ...
FORMS = ("upload", "build", "plain", "guarded-refit", "guarded-rebuild", "sparse", "pose", "pose-guarded-refit", "pose-guarded-rebuild", "bind", "skin",
         "skin-guarded-refit", "skin-guarded-rebuild")
REBUILDS = ("guarded-rebuild", "pose-guarded-rebuild", "skin-guarded-rebuild")
# ... and the pairs no context can make, each with the sentence of include/rvpt_hip.h that rules it out
UNMAKEABLE = {
    ("upload", "guarded-rebuild"): "After an ordinary upload with the caller's own nodes the library has no builder to name: a limit there is RVPT_HIP_ERR_INVALID",
    ("upload", "pose-guarded-rebuild"): "from an ordinary upload with the caller's own nodes is RVPT_HIP_ERR_INVALID",
    ("upload", "skin"): "The binding is DROPPED by an ordinary full upload, by a build form the caller asks for",
    ("build", "skin"): "The binding is DROPPED by an ordinary full upload, by a build form the caller asks for",
    # the guarded skin update is the skin update first: "Every refusal of the skin update comes first", and without a binding that is "skin update before a bind"
    ("upload", "skin-guarded-refit"): "The binding is DROPPED by an ordinary full upload, by a build form the caller asks for",
    ("build", "skin-guarded-refit"): "The binding is DROPPED by an ordinary full upload, by a build form the caller asks for",
    ("upload", "skin-guarded-rebuild"): "The binding is DROPPED by an ordinary full upload, by a build form the caller asks for",  # (and no builder to name)
    ("build", "skin-guarded-rebuild"): "The binding is DROPPED by an ordinary full upload, by a build form the caller asks for",
}
SITUATIONS = ("a guarded plain rebuild while a binding and a rest pose are held, then a skin update",
              "a guarded pose rebuild, then a pose of an unlisted part",
              "a refusal directly after a guarded plain rebuild",
              "a bind between two pose updates",
              "a refusal directly after a guarded pose rebuild",
              "a refusal directly after a guarded skin rebuild",
              "a guarded skin rebuild, then a sparse update",
              "a guarded skin rebuild, then a pose of some parts",
              "a guarded skin rebuild, then a plain skin update with the same bones",
              "a guarded plain rebuild between two guarded skin steps")
# the refusals the generator draws: what, the pattern a message must match — each a piece of the header's wording or of rvpt_abi.hip's and rvpt_scene.hip's message text
REFUSALS = {
    "skin without a binding": "skin update before a bind",
    "skin with too few bones": "the binding names bone",
    "a limit on a caller's tree": "guarded update with a limit after an ordinary upload_scene",
    "a limit on a caller's tree (pose)": "guarded pose update with a limit after an ordinary upload_scene",
    "a limit on a caller's tree (skin)": "guarded skin update with a limit after an ordinary upload_scene",
    "a guarded skin update with a limit on a caller's tree, without a binding": "skin update before a bind",  # the skin update's refusals come first
    "two pose ranges share a triangle": "share triangle",
    "an index twice in a sparse list": "occurs more than once in the list",
    "a plain update of another n_tris": "the uploaded scene has",
    "a bind of the wrong count": "bind for",
}


class Refused(Exception):
    """the header refuses the call: `pattern` is a regular expression the library's message matches"""

    def __init__(self, pattern):
        super().__init__(pattern)
        self.pattern = pattern


class Report(NamedTuple):
    cost: float
    base: float
    rebuilt: bool
    tree: Optional[str]
    new_base: Optional[float]


def numpy_tree(method, tris):
    """(nodes, perm, the tree the call reports) of the numpy statement of a build form"""
    if method == "ploc":
        info = {}
        nodes, perm = scene.build_ploc(tris, info=info)
        return nodes, np.asarray(perm, dtype=np.int64), info["tree"]
    nodes, perm = (scene.build_sah if method == "sah" else scene.build_lbvh)(tris)[:2]
    return nodes, np.asarray(perm, dtype=np.int64), method


def listed_of(moves) -> np.ndarray:
    return gp.listed_of(moves)


def wide_map_of(wide, dev_nodes, shift):
    """d_wide_map for a FRESH wide form, from the form itself: wide node 0 stands for the root; the used slots of a wide node are an expansion of its binary
    node's child list [left, right] (inner entries replaced in place by their two children); of the few expansions of that length the one is taken whose
    leaves carry the slots' leaf heads, whose inner entries sit in slots with wide indices, and whose boxes are the slots' bytes.  ValueError where two fit."""
    n_wide = wide.shape[0]
    out = np.full((n_wide, 4), EMPTY, dtype=np.uint32)
    if n_wide == 0:
        return out
    heads = wide[:, 6, :].view(np.uint32)
    first, count = dev_nodes["first"].astype(np.int64), dev_nodes["count"].astype(np.int64)
    box = np.ascontiguousarray(dev_nodes["bounds"]).view(np.uint32)
    slot_box = np.ascontiguousarray(np.transpose(wide[:, :6, :], (0, 2, 1))).view(np.uint32)  # [wide, slot, 6]
    binary_of = np.full(n_wide, -1, dtype=np.int64)
    binary_of[0] = 0

    def expansions(lst, k):
        if len(lst) == k:
            yield tuple(lst)
        elif len(lst) < k:
            for i, node in enumerate(lst):
                if count[node] == 0:
                    yield from expansions(lst[:i] + [int(first[node]), int(first[node]) + 1] + lst[i + 1:], k)

    for wi in range(n_wide):
        b = int(binary_of[wi])
        k = int((heads[wi] != EMPTY).sum())
        fits = set()
        for cand in set(expansions([int(first[b]), int(first[b]) + 1], k)):
            ok = True
            for s, node in enumerate(cand):
                h = int(heads[wi, s])
                leaf_head = int(first[node]) | (int(count[node]) << shift)
                if (h != leaf_head if count[node] > 0 else h >= n_wide) or not np.array_equal(slot_box[wi, s], box[node]):
                    ok = False
                    break
            if ok:
                fits.add(cand)
        if len(fits) != 1:
            raise ValueError(f"wide_map_of: {len(fits)} expansions of binary node {b} fit wide node {wi}")
        cand = fits.pop()
        out[wi, :k] = cand
        for s, node in enumerate(cand):
            if count[node] == 0:
                binary_of[int(heads[wi, s])] = node
    return out


class Model:
    """what one context holds of its geometry; bvh=False: a brute-force context, the same model without the tree parts"""

    def __init__(self, bvh=True):
        self.bvh = bvh
        self.nodes = None        # the tree in the layout its maker gave it: a numpy builder's, or the caller's
        self.perm = None         # stored position -> caller's index; None after an ordinary upload
        self.built_by = None     # None, "lbvh", "ploc", "sah": the builder a rebuild runs ("ploc" after a PLOC build that fell back, as the read-back says)
        self.tree = None         # the name of the tree the scene then holds
        self.base_cost = None
        self.current = None      # float32[n, 16] in update order
        self.rest = None         # float32[n, 16] in update order, or None where the context holds no rest pose
        self.binding = None      # VERTEX_SKIN_DTYPE[3 n] in update order, or None
        self.max_bone = None
        self.have_sparse_maps = False
        self.have_inv_perm = False
        self.exp = None          # ds.Expected of the tree as the last upload, build or rebuild left it: topology, level table, head shift, maps
        self.wide = None         # the wide form: exp.wide for a fresh tree, ds.regathered afterwards — the grouping is the fresh one's
        self.wide_map = None

    def copy(self):
        return copy.copy(self)

    @property
    def n(self):
        return 0 if self.current is None else self.current.shape[0]

    def stored(self, rows=None):
        rows = self.current if rows is None else rows
        return rows if self.perm is None else rows[self.perm]

    def inverse(self):
        inv = np.empty(self.n, dtype=np.int64)
        inv[self.perm] = np.arange(self.n)
        return inv

    def positions(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        return idx if self.perm is None else self.inverse()[idx]

    def device_nodes(self):
        """d_nodes: upload_scene's layout of the tree as it stands"""
        return ds.shifted_layout(self.nodes) if self.perm is not None else ds.device_layout(self.nodes)[0]

    # ---- what replaces the tree ------------------------------------------------------------------------------------------------------------------------------

    def _fresh_tree(self, nodes, perm, built_by, tree):
        self.nodes = np.ascontiguousarray(nodes).view(ds.NODE).reshape(-1).copy()
        self.perm, self.built_by, self.tree = perm, built_by, tree
        self.base_cost = scene.tree_cost(self.nodes)
        self.exp = ds.Expected(self.nodes, breadth_first=perm is not None)
        self.wide = self.exp.wide
        self.wide_map = wide_map_of(self.exp.wide, self.exp.nodes, self.exp.head_shift)
        self.have_sparse_maps = self.have_inv_perm = False  # "dropped by every full upload, build and rebuild"

    def _refit(self, touched=None):
        self.nodes = scene.refit_bvh(self.nodes, self.stored(), touched=touched)
        self.wide = ds.regathered(self.wide, self.wide_map, self.device_nodes())  # "the 4-wide form keeps the grouping the upload made, as after every update form"

    def upload(self, nodes, tris):
        """the ordinary upload: the caller's nodes (None on a brute-force context) over triangles in leaf order; drops the rest pose and the binding"""
        self.current = np.array(tris, dtype=np.float32).reshape(-1, 16)
        self.rest = self.binding = self.max_bone = None
        if self.bvh:
            self._fresh_tree(nodes, None, None, None)
        return None

    def build(self, method, tris):
        """a build form the caller asks for: the builder's tree over the triangles in the caller's order; drops the rest pose and the binding.  Brute-force
        contexts ignore the count: the ordinary upload."""
        self.current = np.array(tris, dtype=np.float32).reshape(-1, 16)
        self.rest = self.binding = self.max_bone = None
        if self.bvh:
            nodes, perm, tree = numpy_tree(method, self.current)
            self._fresh_tree(nodes, perm, method, tree)
        return None

    def _rebuild(self):
        """a rebuild the library makes itself: by the builder that made the tree, from the vertices as they stand beside the stored mat_id rows, in the
        caller's order; the binding survives, the maps go"""
        nodes, perm, tree = numpy_tree(self.built_by, self.current)
        self._fresh_tree(nodes, perm, self.built_by, tree)

    # ---- the update forms ------------------------------------------------------------------------------------------------------------------------------------

    def _take_vertices(self, tris):
        tris = np.asarray(tris, dtype=np.float32).reshape(-1, 16)
        if tris.shape[0] != self.n:
            raise Refused(REFUSALS["a plain update of another n_tris"])
        return tris

    def _moved(self, tris):
        out = self.current.copy()
        out[:, :12] = tris[:, :12]  # "only the twelve floats vert0..vert2 of every triangle are taken"; the stored mat_id rows are kept
        self.current, self.rest = out, None  # a successful call of another form: the next pose update takes a fresh snapshot
        if self.bvh:
            self._refit()

    def update(self, tris):
        self._moved(self._take_vertices(tris))
        return None

    def update_guarded(self, tris, limit):
        """limit: a factor (1000 .. 65535 thousandths) or math.inf / None, report only"""
        permille = gp.permille_of(limit)
        tris = self._take_vertices(tris)  # "with the update form's own messages"
        if not self.bvh:  # "there the guarded count is the plain update form"
            self._moved(tris)
            return None
        if permille != 0 and self.built_by is None:
            raise Refused(REFUSALS["a limit on a caller's tree"])
        self._moved(tris)
        cost, base = scene.tree_cost(self.nodes), self.base_cost
        if permille == 0 or not cost > permille / 1000.0 * base:
            return Report(cost, base, False, None, None)
        self._rebuild()
        return Report(cost, base, True, self.built_by, self.base_cost)  # (this form's sentence names the builder)

    def update_sparse(self, idx, rows):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 16)
        if idx.shape[0] > self.n:
            raise Refused("sparse update with")
        if idx.size and (idx.min() < 0 or idx.max() >= self.n):
            raise Refused("is outside the")
        if np.unique(idx).shape[0] != idx.shape[0]:
            raise Refused(REFUSALS["an index twice in a sparse list"])
        out = self.current.copy()
        out[idx, :12] = rows[:, :12]
        self.current, self.rest = out, None
        if self.bvh:
            self._refit(touched=self.positions(idx))
            self.have_sparse_maps, self.have_inv_perm = True, self.perm is not None
        return None

    def _check_moves(self, moves):
        rec = scene.part_moves(moves)
        taken = np.zeros(self.n, dtype=bool)
        for r in rec:
            first, count = int(r["first"]), int(r["count"])
            if count == 0:
                raise Refused("pose update")
            if first + count > self.n:
                raise Refused("pose update")
            if taken[first:first + count].any():
                raise Refused(REFUSALS["two pose ranges share a triangle"])
            taken[first:first + count] = True
        return rec

    def _pose(self, rec):
        if self.rest is None:
            self.rest = self.current  # the snapshot: the stored vertices as the last call of any other form left them, earlier poses included
        self.current = scene.pose_parts(self.rest, rec, current=self.current)  # always from the rest pose; a part not listed keeps the pose it has
        if self.bvh:
            self._refit(touched=self.positions(listed_of(rec)))
            self.have_sparse_maps, self.have_inv_perm = True, self.perm is not None

    def pose(self, moves):
        self._pose(self._check_moves(moves))
        return None

    def pose_guarded(self, moves, limit):
        permille = gp.permille_of(limit)
        rec = self._check_moves(moves)  # "every refusal of the pose update comes first"
        if not self.bvh:
            self._pose(rec)
            return None
        if permille != 0 and self.built_by is None:
            raise Refused(REFUSALS["a limit on a caller's tree (pose)"])
        self._pose(rec)
        cost, base = scene.tree_cost(self.nodes), self.base_cost
        if permille == 0 or not cost > permille / 1000.0 * base:
            return Report(cost, base, False, None, None)
        rest = self.rest
        self._rebuild()  # THE REST POSE GOES WITH THE REBUILD: in update order it is the same array
        self.rest = rest
        return Report(cost, base, True, self.tree, self.base_cost)  # (this form's sentence names the tree the scene then holds)

    def bind(self, records):
        rec = scene.vertex_skins(records)
        if rec.shape[0] != 3 * self.n:
            raise Refused(REFUSALS["a bind of the wrong count"])
        if rec.size and int(rec["bone"].max()) >= scene.SKIN_MAX_BONES:
            raise Refused("a bone index lies below")
        self.binding = rec.copy()  # it moves nothing and is not "another form": the rest pose stays
        self.max_bone = int(rec["bone"].max()) if rec.size else 0
        return None

    def _check_bones(self, bones):
        m = scene.bone_matrices(bones)
        if self.binding is None:
            raise Refused(REFUSALS["skin without a binding"])
        if m.shape[0] <= self.max_bone:
            raise Refused(REFUSALS["skin with too few bones"])
        return m

    def _skin(self, m):
        if self.rest is None:
            self.rest = self.current
        self.current = scene.skin_triangles(self.rest, self.binding, m)  # every triangle, from the rest pose, which it keeps
        if self.bvh:
            self._refit()  # "every box is then refitted by the PLAIN form's rule"

    def skin(self, bones):
        self._skin(self._check_bones(bones))
        return None

    def skin_guarded(self, bones, limit):
        permille = gp.permille_of(limit)
        m = self._check_bones(bones)  # "every refusal of the skin update comes first, in its words and its order"
        if not self.bvh:  # "there the count is the plain skin update"
            self._skin(m)
            return None
        if permille != 0 and self.built_by is None:  # "then the one refusal of this form"; "report only (0) is legal there"
            raise Refused(REFUSALS["a limit on a caller's tree (skin)"])
        self._skin(m)
        cost, base = scene.tree_cost(self.nodes), self.base_cost
        if permille == 0 or not cost > permille / 1000.0 * base:
            return Report(cost, base, False, None, None)
        rest = self.rest
        self._rebuild()  # THE REST POSE GOES WITH THE REBUILD, THE BINDING STAYS WHERE IT IS: in update order both are the same arrays, and max_bone stays
        self.rest = rest
        return Report(cost, base, True, self.tree, self.base_cost)  # (the tree the scene then holds: a PLOC rebuild that fell back names lbvh)

    # ---- the read-back ---------------------------------------------------------------------------------------------------------------------------------------

    def differences(self, state, brute_pieces=("tris", "rest", "skin")):
        """Context.scene_state() against the model, byte for byte: a list of (piece, detail), empty where the device holds what the model states"""
        out = []

        def same(name, got, want, nodes=False):
            if not (ds.same_nodes(got, want) if nodes else ds.same_bytes(got, want)):
                out.append((name, ds.first_difference(got, want)))

        same("tris", state["tris"], self.stored())
        same("rest", state["rest"], np.zeros((0, 12), np.float32) if self.rest is None else self.stored(self.rest)[:, :12])
        if self.binding is None:
            if state["skin"].size:
                out.append(("skin", "the device holds a binding, the model none"))
        elif state["skin"].tobytes() != self.binding.tobytes():
            out.append(("skin", ds.first_difference(state["skin"].view(np.uint8).reshape(-1, 32), self.binding.view(np.uint8).reshape(-1, 32))))
        if not self.bvh:
            return out
        exp, dev = self.exp, self.device_nodes()
        same("nodes", state["nodes"], dev, nodes=True)
        same("perm", state["perm"], np.zeros(0, np.uint32) if self.perm is None else self.perm.astype(np.uint32))
        same("wide", state["wide"], self.wide)
        same("wide_map", state["wide_map"], self.wide_map)
        same("refit_levels", state["refit_levels"], exp.levels)
        for name, want in (("bvh_height", exp.height), ("bvh_head_shift", exp.head_shift), ("n_nodes", exp.n_nodes), ("n_tris", exp.n_tris), ("n_wide", self.wide.shape[0]),
                           ("wide_stack_levels", exp.wide_stack_levels), ("built_by", self.built_by), ("have_perm", self.perm is not None),
                           ("have_sparse_maps", self.have_sparse_maps), ("have_inv_perm", self.have_inv_perm), ("have_cost", True)):
            if state[name] != want:
                out.append((name, (state[name], want)))
        same("inv_perm", state["inv_perm"], self.inverse().astype(np.uint32) if self.have_inv_perm else np.zeros(0, np.uint32))
        if self.have_sparse_maps:
            same("sparse_parent", state["sparse_parent"], exp.parent[:exp.n_map_nodes])
            same("sparse_leaf_of", state["sparse_leaf_of"], exp.leaf_of)
            if state["sparse_dirty"].shape != (exp.n_map_nodes,):
                out.append(("sparse_dirty", state["sparse_dirty"].shape))
        else:
            for name in ("sparse_parent", "sparse_leaf_of", "sparse_dirty"):
                if state[name].size:
                    out.append((name, "held without maps"))
        if state["sparse_dirty"].any():
            out.append(("sparse_dirty", np.flatnonzero(state["sparse_dirty"])[:8]))
        try:
            ds.check_wide_map(state, "d_wide_map")
        except AssertionError as e:
            out.append(("wide_map structure", str(e)))
        return out


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------------------------------

SCENE_NAMES = ("soup257", "lattice600", "default143", "cornell1")
_SCENES = {}


def without_zeros(tris):
    """the triangles moved as a whole, by an offset that is no coordinate's negative, until no vertex coordinate is 0 (the default and the Cornell scene have
    vertices on the coordinate planes); float32 throughout"""
    t = np.array(tris, dtype=np.float32)
    v = ds.vertices(t)
    offset = np.float32(0.0)
    while (v + offset == 0).any():
        offset += np.float32(0.03125 + 1.0 / 1024.0)
    v += offset
    return t


def scene_of(name):
    """(triangles float32[n, 16] in a caller's order, materials): built once, shared, read-only; at most MAX_TRIS triangles, no zero coordinate"""
    if name not in _SCENES:
        if name == "soup257":
            tris, mats = ds.soup(257, 257), scene.default_materials()
        elif name == "lattice600":
            tris, mats = ds.lattice(600, 600), scene.default_materials()
        elif name == "default143":
            tris, mats = scene.default_scene()
            tris = without_zeros(tris)
        else:
            tris, mats = scene.cornell_scene(1)
            tris = without_zeros(tris)[np.random.RandomState(17).permutation(tris.shape[0])]
        tris, mats = np.ascontiguousarray(tris, dtype=np.float32), np.ascontiguousarray(mats, dtype=np.float32)
        assert tris.shape[0] <= MAX_TRIS and ds.no_zero_coordinate(tris), name
        for a in (tris, mats):
            a.setflags(write=False)
        _SCENES[name] = (tris, mats)
    return _SCENES[name]


def extent(tris):
    return float(np.ptp(ds.vertices(tris).reshape(-1, 3), axis=0).max())


# ---- the steps ---------------------------------------------------------------------------------------------------------------------------------------------------

class Step(NamedTuple):
    form: str                # the Model method, and the wrapper's form
    args: tuple              # what the method takes: numpy arrays, a builder's name, a limit
    on_device: bool          # the arrays go down as torch tensors on the context's device (only where the header allows device memory)
    kind: str                # one of FORMS, or "refusal: " + a key of REFUSALS
    pattern: Optional[str]   # a refusal's pattern
    held: tuple              # (a binding is held, a rest pose is held) BEFORE the step

    @property
    def refusal(self):
        return self.pattern is not None


def apply(model, step):
    """the step on the model: what the call reports; Refused passes through"""
    return getattr(model, step.form)(*step.args)


def step_bytes(step) -> bytes:
    parts = [step.form.encode(), step.kind.encode(), bytes([step.on_device])]
    for a in step.args:
        parts.append(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else repr(a).encode())
    return b"|".join(parts)


def ranges_of(step):
    return listed_of(step.args[0]) if step.form in ("pose", "pose_guarded") else None


class _Draw:
    """the motions and lists of one sequence, drawn from its own RandomState"""

    def __init__(self, rng, model):
        self.rng, self.m = rng, model

    def phase(self):
        return float(self.rng.uniform(0.0, 6.0))

    def part(self, avoid=None):
        """(first, count): sizes straddle a wave of 64; avoid: triangles the range must not hold"""
        n = self.m.n
        for _ in range(64):
            count = int(min(n, self.rng.choice([1, 63, 64, 65, max(1, n // 10), max(1, n // 3)])))
            first = int(self.rng.randint(0, n - count + 1))
            if avoid is None or not np.intersect1d(np.arange(first, first + count), avoid).size:
                return first, count
        free = np.setdiff1d(np.arange(n), avoid)
        if free.size == 0:
            raise ValueError("no free part")
        return int(free[self.rng.randint(free.size)]), 1

    def small_motion(self, rows, first, count):
        """a rotation of a few degrees about the part's centroid and an offset of a few percent of the extent"""
        f, c, m = gp.turned(rows, first, count, float(self.rng.uniform(-4.0, 4.0)))
        m = m.copy()
        m[:, 3] += self.rng.uniform(-0.03, 0.03, 3) * extent(rows)
        return (f, c, m)

    def carried(self, rows, first, count, attempt):
        f, c, m = gp.carried(rows, first, count)
        m = m.copy()
        m[:, 3] *= (1.0 + attempt) * (1.0 if self.rng.rand() < 0.5 else -1.0)
        return (f, c, m)

    def wobbled(self):
        out = scene.wobble(self.m.current, self.phase(), 0.02 * extent(self.m.current))
        if self.rng.rand() < 0.5:
            out[:, 12:] = 77.0  # the material row of the source is not read
        return out

    def carried_triangles(self, attempt):
        first, count = self.part()
        return scene.pose_parts(self.m.current, [self.carried(self.m.current, first, count, attempt)])

    def moves(self, avoid=None, carry=False, attempt=0):
        """one to four disjoint parts; an identity pose and a whole-mesh part are among them"""
        rows = self.m.current if self.m.rest is None else self.m.rest
        n = self.m.n
        if not carry and avoid is None and self.rng.rand() < 0.15:
            return scene.part_moves([self.small_motion(rows, 0, n)])  # the whole mesh as one part
        k = int(self.rng.randint(1, 5))
        out, taken = [], (np.zeros(0, np.int64) if avoid is None else np.asarray(avoid))
        for p in range(k):
            try:
                first, count = self.part(avoid=taken if taken.size else None)
            except ValueError:
                break
            taken = np.concatenate([taken, np.arange(first, first + count)])
            if carry and p == 0:
                out.append(self.carried(rows, first, count, attempt))
            elif self.rng.rand() < 0.2:
                out.append((first, count, np.eye(3, 4)))  # an identity pose
            else:
                out.append(self.small_motion(rows, first, count))
        return scene.part_moves(out)

    def sparse(self):
        """(indices, rows): a single index, a contiguous block, a scatter, all triangles shuffled"""
        n = self.m.n
        which = int(self.rng.randint(4))
        if which == 0:
            idx = np.array([self.rng.randint(n)])
        elif which == 1:
            first, count = self.part()
            idx = np.arange(first, first + count)
        elif which == 2:
            idx = self.rng.permutation(n)[:max(2, n // 7)]
        else:
            idx = self.rng.permutation(n)
        rows = scene.wobble(self.m.current, self.phase(), 0.03 * extent(self.m.current))[idx]
        return idx.astype(np.int64), np.ascontiguousarray(rows)

    def binding(self, many=False):
        """many: enough bones that a block of them can be carried away from its neighbours (tests/_guarded_skin.py: carried_bones)"""
        return _skin.weights(self.m.current if self.m.rest is None else self.m.rest, int(self.rng.choice([16, 64] if many else [1, 3, 16, 64])))

    def bones(self, k=None):
        rows = self.m.current if self.m.rest is None else self.m.rest
        return _skin.bones(rows, self.m.max_bone + 1 if k is None else k, self.phase())

    def carrying(self, attempt):
        """tests/_guarded_skin.py's carrying set for the bones bound: gentle rotations, the blocks of carried_bones translated along an axis — another axis,
        sign and length with every attempt, as carried_triangles varies its motion"""
        rows = self.m.current if self.m.rest is None else self.m.rest
        k = self.m.max_bone + 1
        axis = gs.axes_by_extent(rows)[(attempt + int(self.rng.randint(3))) % 3]
        out = gs.carrying(rows, k, axis, self.phase())
        factor = (1.0 + attempt // 3) * (1.0 if self.rng.rand() < 0.5 else -1.0)
        for b in gs.carried_bones(k):
            out[b, axis, 3] += np.float32((factor - 1.0) * 0.5 * extent(rows))
        return out

    def caller_tree(self, loose):
        """the caller's own tree over the triangles as they stand: (nodes, triangles in leaf order)"""
        nodes, order = native.build_bvh(np.ascontiguousarray(self.m.current))
        nodes = np.ascontiguousarray(nodes).view(ds.NODE).reshape(-1)
        if loose:
            from test_gpu_parity import _loosen_boxes
            nodes = _loosen_boxes(nodes, int(self.rng.randint(1 << 30)))
        return nodes, np.ascontiguousarray(self.m.current[order])


def _guard_limit(rng, ratio, rebuild, built):
    """a limit for a guarded step whose tree costs `ratio` x base: one that rebuilds, one that does not, or report only (math.inf); None where there is none"""
    if rebuild:
        top = min(65535, int(math.floor(ratio * 1000.0 * 0.98)))
        return None if top < 1000 else int(rng.randint(1000, top + 1)) / 1000.0
    if not built or rng.rand() < 0.4:
        return math.inf
    low = max(1000, int(math.ceil(ratio * 1000.0 * 1.02)))
    return math.inf if low > 65535 else int(min(65535, low + rng.randint(0, 300))) / 1000.0


def _clear_of_limit(report, limit):
    permille = gp.permille_of(limit)
    return permille == 0 or report.base == 0 or abs(report.cost / (permille / 1000.0 * report.base) - 1.0) > MARGIN


def _available(model, prev_listed):
    kinds = ["pose", "pose-guarded-refit", "bind", "plain", "guarded-refit", "sparse", "upload", "build"]
    if model.binding is not None:
        kinds += ["skin", "skin-guarded-refit"]
    if model.bvh and model.built_by is not None:
        kinds += ["guarded-rebuild", "pose-guarded-rebuild"]
        if model.binding is not None:
            kinds.append("skin-guarded-rebuild")
    return kinds


def _refusals_available(model):
    out = ["two pose ranges share a triangle", "an index twice in a sparse list", "a plain update of another n_tris", "a bind of the wrong count"]
    if model.binding is None:
        out.append("skin without a binding")
    elif model.max_bone >= 1:
        out.append("skin with too few bones")
    if model.bvh and model.built_by is None:
        out += ["a limit on a caller's tree", "a limit on a caller's tree (pose)"]
        out.append("a limit on a caller's tree (skin)" if model.binding is not None else "a guarded skin update with a limit on a caller's tree, without a binding")
    return out


def _draw_refusal(draw, what):
    m, rng = draw.m, draw.rng
    if what == "skin without a binding":
        return "skin", (_skin.bones(m.current, 3, draw.phase()),)
    if what == "skin with too few bones":
        return "skin", (draw.bones(k=m.max_bone),)
    if what == "a limit on a caller's tree":
        return "update_guarded", (draw.wobbled(), 1.0 + int(rng.randint(0, 500)) / 1000.0)
    if what == "a limit on a caller's tree (pose)":
        return "pose_guarded", (draw.moves(), 1.0 + int(rng.randint(0, 500)) / 1000.0)
    if what == "a limit on a caller's tree (skin)":
        return "skin_guarded", (draw.bones(), 1.0 + int(rng.randint(0, 500)) / 1000.0)
    if what == "a guarded skin update with a limit on a caller's tree, without a binding":
        return "skin_guarded", (_skin.bones(m.current, 3, draw.phase()), 1.0 + int(rng.randint(0, 500)) / 1000.0)
    if what == "two pose ranges share a triangle":
        rec = draw.moves()
        first, count = int(rec["first"][-1]), int(rec["count"][-1])
        extra = scene.part_moves([(first + count - 1, 1, np.eye(3, 4))])
        return "pose", (np.concatenate([rec, extra]),)
    if what == "an index twice in a sparse list":
        idx, rows = draw.sparse()
        if idx.shape[0] == m.n:  # (one more than the scene holds would be the earlier refusal)
            idx, rows = idx[:-1], rows[:-1]
        return "update_sparse", (np.concatenate([idx, idx[:1]]), np.concatenate([rows, rows[:1]]))
    if what == "a plain update of another n_tris":
        t = draw.wobbled()
        return "update", (np.ascontiguousarray(t[:-1]) if rng.rand() < 0.5 else np.concatenate([t, t[:1]]),)
    assert what == "a bind of the wrong count"
    return "bind", (draw.binding()[:-3].copy(),)


DEVICE_FORMS = ("build", "update", "update_guarded", "update_sparse", "bind", "skin", "skin_guarded")  # where the header allows device memory; a pose list is host memory


def _draw_kind(draw, kind, prev_listed, attempt):
    """(form, args) for a step meant to be of `kind`; the generator checks what the model makes of it"""
    m, rng = draw.m, draw.rng
    if kind == "upload":
        return "upload", ((None, np.ascontiguousarray(m.current)) if not m.bvh else draw.caller_tree(loose=rng.rand() < 0.4))
    if kind == "build":
        methods = BUILDERS if m.bvh else BUILDERS[:2]  # (on a brute-force context the wrapper takes the two older names, and ignores them)
        return "build", (str(rng.choice(methods)) if m.built_by is None or rng.rand() < 0.4 else m.built_by, np.ascontiguousarray(m.current))
    if kind == "plain":
        return "update", (draw.wobbled(),)
    if kind == "sparse":
        return "update_sparse", draw.sparse()
    if kind == "bind":
        return "bind", (draw.binding(),)
    if kind == "bind-many":
        return "bind", (draw.binding(many=True),)
    if kind == "skin":
        return "skin", (draw.bones(),)
    if kind == "pose":
        return "pose", (draw.moves(avoid=prev_listed),)
    rebuild = kind.endswith("rebuild")
    if kind.startswith("pose-guarded"):
        args = (draw.moves(carry=rebuild, attempt=attempt),)
        form = "pose_guarded"
    elif kind.startswith("skin-guarded"):
        if rebuild and one_bone(m.binding):
            return None  # one bone carries the whole mesh along: no tree gets worse by that
        args = (draw.carrying(attempt) if rebuild else draw.bones(),)
        form = "skin_guarded"
    else:
        args = (draw.carried_triangles(attempt) if rebuild else draw.wobbled(),)
        form = "update_guarded"
    trial = m.copy()
    report = getattr(trial, form)(*args, math.inf)
    if report is None:  # a brute-force context: the plain form, any limit
        return form, args + (math.inf if rng.rand() < 0.5 else 1.25,)
    limit = _guard_limit(rng, report.cost / report.base if report.base > 0 else 0.0, rebuild, m.built_by is not None)
    return (form, args + (limit,)) if limit is not None else None


def one_bone(binding) -> bool:
    """every influence that counts names the same bone: the skin update is then one pose of the whole mesh"""
    return np.unique(binding["bone"][binding["weight"] != 0]).size <= 1


def rebuild_conditions(before, after):
    """what a skin-guarded-rebuild step of the suite must be for a wrong device to show, as a list of what fails: the rebuild changes the permutation (or the
    rest pose carried by the old one would still fit), the rest pose is not the skinned pose (or carrying the wrong one would not show), and the binding is
    not one pose of the whole mesh (or a binding read through the wrong permutation would skin alike)"""
    out = []
    if np.array_equal(before.perm, after.perm):
        out.append("the permutation stays")
    if after.rest.tobytes() == after.current.tobytes():
        out.append("the rest pose is the skinned pose")
    if one_bone(after.binding):
        out.append("the binding names one bone")
    return out


def kind_of(step_form, report, pattern=None):
    if step_form in ("upload", "build", "bind", "skin", "pose"):
        return step_form
    if step_form == "update":
        return "plain"
    if step_form == "update_sparse":
        return "sparse"
    prefix = {"update_guarded": "guarded", "pose_guarded": "pose-guarded", "skin_guarded": "skin-guarded"}[step_form]
    return f"{prefix}-{'rebuild' if report is not None and report.rebuilt else 'refit'}"


# the named situations, in one walk: what a token makes beyond its kind is said in ALIAS
SCRIPT = ("bind-many", "skin", "guarded-rebuild", "skin", "pose-guarded-rebuild", "pose-unlisted", "bind-many", "pose", "skin-guarded-rebuild", "sparse",
          "skin-guarded-rebuild", "refusal", "skin-guarded-rebuild", "pose", "skin-guarded-rebuild", "skin-same", "skin-guarded-refit", "guarded-rebuild",
          "skin-guarded-refit", "guarded-rebuild", "refusal", "pose-guarded-rebuild", "refusal")
ALIAS = {"bind-many": "bind",       # a bind of 16 or 64 bones
         "pose-unlisted": "pose",   # a pose that avoids the parts the guarded pose rebuild before it listed
         "skin-same": "skin"}       # the plain skin update with the bones of the guarded skin update before it


class Coverage:
    """what the sequences generated so far have covered: the greedy choice steers by it"""

    def __init__(self):
        self.pairs = {}
        self.refusals = {k: 0 for k in REFUSALS}
        self.situations = {b: set() for b in BUILDERS}

    def count(self, steps, source=None):
        for a, b in zip(steps, steps[1:]):
            if not a.refusal and not b.refusal:
                self.pairs[a.kind, b.kind] = self.pairs.get((a.kind, b.kind), 0) + 1
        for s in steps:
            if s.refusal:
                self.refusals[s.kind[len("refusal: "):]] += 1
        if source in BUILDERS:
            self.situations[source] |= situations_in(steps)

    def missing(self):
        return sorted((a, b) for a in FORMS for b in FORMS if (a, b) not in UNMAKEABLE and (a, b) not in self.pairs)

    def table(self):
        lines = ["pairs of neighbouring successful steps (row: the first, column: the second; '-': no context can make it)",
                 " " * 22 + " ".join(f"{k[:7]:>7}" for k in FORMS)]
        for a in FORMS:
            lines.append(f"{a:>22}" + " ".join(f"{'-' if (a, b) in UNMAKEABLE else self.pairs.get((a, b), 0):>7}" for b in FORMS))
        lines.append("refusals: " + ", ".join(f"{k} {v}" for k, v in self.refusals.items()))
        for b in BUILDERS:
            lines.append(f"situations, {b}: " + "; ".join(f"{'yes' if s in self.situations[b] else 'NO'}: {s}" for s in SITUATIONS))
        return "\n".join(lines)


def situations_in(steps):
    found = set()
    for i, s in enumerate(steps):
        nxt = steps[i + 1] if i + 1 < len(steps) else None
        if nxt is None:
            break
        if s.kind == "guarded-rebuild" and s.held == (True, True) and nxt.kind == "skin":
            found.add(SITUATIONS[0])
        if s.kind == "pose-guarded-rebuild" and nxt.form in ("pose", "pose_guarded") and not nxt.refusal and not np.intersect1d(ranges_of(s), ranges_of(nxt)).size:
            found.add(SITUATIONS[1])
        if s.kind in REBUILDS and nxt.refusal:
            found.add(SITUATIONS[{"guarded-rebuild": 2, "pose-guarded-rebuild": 4, "skin-guarded-rebuild": 5}[s.kind]])
        if s.kind == "skin-guarded-rebuild" and nxt.kind == "sparse":
            found.add(SITUATIONS[6])
        if s.kind == "skin-guarded-rebuild" and nxt.kind == "pose":
            found.add(SITUATIONS[7])
        if s.kind == "skin-guarded-rebuild" and nxt.kind == "skin" and np.asarray(nxt.args[0]).tobytes() == np.asarray(s.args[0]).tobytes():
            found.add(SITUATIONS[8])
        if s.kind == "guarded-rebuild" and i > 0 and steps[i - 1].kind.startswith("skin-guarded") and nxt.kind.startswith("skin-guarded"):
            found.add(SITUATIONS[9])
        if s.kind == "bind" and i > 0 and steps[i - 1].kind.startswith("pose") and nxt.kind.startswith("pose") and not nxt.refusal:
            found.add(SITUATIONS[3])
    return found


def sequence(seed, source, n_steps, coverage=None):
    """[Step] * n_steps, the first of which makes the scene by `source`.  Reproducible: the same (seed, source, n_steps) and the same coverage so far give the
    same bytes.  Every step leaves no zero coordinate, and every guarded step with a limit has cost / (limit x base) further than MARGIN from 1: the generator
    redraws the motion or the limit, REDRAWS times at the most, and takes another form where that does not help — no step is dropped."""
    assert source in SOURCES and 1 <= n_steps
    coverage = Coverage() if coverage is None else coverage
    pairs = dict(coverage.pairs)
    refusals = dict(coverage.refusals)
    rng = np.random.RandomState([int(seed), SOURCES.index(source)])
    tris, _ = scene_of(SCENE_NAMES[int(seed) % len(SCENE_NAMES)])
    model = Model(bvh=source != "brute")
    draw = _Draw(rng, model)
    model.current = tris  # (what caller_tree reads)
    if source in BUILDERS:
        first = Step("build", (source, tris), bool(rng.rand() < 0.5), "build", None, (False, False))
    elif source == "brute":
        first = Step("upload", (None, tris), False, "upload", None, (False, False))
    else:
        first = Step("upload", draw.caller_tree(loose=source == "upload-loose"), False, "upload", None, (False, False))
    apply(model, first)
    steps = [first]
    script = list(SCRIPT) if source in BUILDERS and len(coverage.situations[source]) < len(SITUATIONS) else []
    prev_listed = None  # the triangles a guarded pose rebuild listed: the next pose avoids them
    while len(steps) < n_steps:
        prev = steps[-1]
        wanted = script.pop(0) if script else None
        rare = min(refusals[o] for o in _refusals_available(model)) < 2  # a refusal met less than twice can be made here: three times as likely
        want_refusal = wanted == "refusal" or (wanted is None and len(steps) > 1 and not prev.refusal and rng.rand() < (3.0 if rare else 1.0) / 8.0)
        held = (model.binding is not None, model.rest is not None)
        if want_refusal:
            options = _refusals_available(model)
            least = min(refusals[o] for o in options)
            what = options[int(rng.randint(len(options)))] if rng.rand() < 0.25 else [o for o in options if refusals[o] == least][0]
            form, args = _draw_refusal(draw, what)
            step = Step(form, args, bool(model.bvh and form in DEVICE_FORMS and rng.rand() < 0.4), "refusal: " + what, REFUSALS[what], held)
            trial = model.copy()
            try:
                apply(trial, step)
                raise AssertionError(f"the model takes what should be refused: {what}")
            except Refused as r:
                assert r.pattern == step.pattern, (what, r.pattern)
            refusals[what] += 1
            steps.append(step)
            continue
        options = _available(model, prev_listed)
        if wanted is not None:
            ranked = [wanted]
        else:
            def score(k):
                new = 0 if prev.refusal else 4 * ((prev.kind, k) not in pairs and (prev.kind, k) not in UNMAKEABLE)
                ahead = sum((k, g) not in pairs and (k, g) not in UNMAKEABLE for g in FORMS) / len(FORMS)
                return new + ahead + 0.5 * rng.rand()
            ranked = sorted(options, key=score, reverse=True)
        ranked += [k for k in ("plain", "sparse") if k not in ranked]  # (what is left where a wanted form cannot be made: always makeable)
        step = None
        for token in ranked:
            kind = ALIAS.get(token, token)
            if kind not in options:
                continue
            for attempt in range(REDRAWS + 1):
                if token == "skin-same":
                    drawn = ("skin", (prev.args[0],)) if prev.form == "skin_guarded" else None
                else:
                    drawn = _draw_kind(draw, token if token == "bind-many" else kind, prev_listed if kind == "pose" and prev.kind == "pose-guarded-rebuild" else None, attempt)
                if drawn is None:
                    continue
                form, args = drawn
                trial = model.copy()
                report = apply(trial, Step(form, args, False, kind, None, held))
                if kind_of(form, report) != kind or not ds.no_zero_coordinate(trial.current):
                    continue
                if report is not None and not _clear_of_limit(report, args[-1]):
                    continue
                if kind == "skin-guarded-rebuild" and rebuild_conditions(model, trial):
                    continue
                step = Step(form, args, bool(model.bvh and form in DEVICE_FORMS and rng.rand() < 0.4), kind, None, held)
                break
            if step is not None:
                break
        assert step is not None, "no form could be drawn"
        apply(model, step)
        draw.m = model
        prev_listed = ranges_of(step) if step.kind == "pose-guarded-rebuild" else None
        if not prev.refusal:
            pairs[prev.kind, step.kind] = pairs.get((prev.kind, step.kind), 0) + 1
        steps.append(step)
    return steps


# ---- the sequences the suite runs ----------------------------------------------------------------------------------------------------------------------------------

class Spec(NamedTuple):
    seed: int
    source: str
    mode: str  # "lab": a laboratory context, read back after every step; "lab-ordered": the same under TRAVERSAL_BVH_ORDERED; "release": no read-back


SUITE = (Spec(1, "upload", "lab"), Spec(2, "upload-loose", "lab"), Spec(3, "lbvh", "lab"), Spec(4, "ploc", "lab"), Spec(5, "sah", "lab"), Spec(6, "lbvh", "lab"),
         Spec(7, "ploc", "lab"), Spec(8, "sah", "lab"), Spec(9, "upload", "lab"), Spec(10, "upload-loose", "lab"), Spec(11, "lbvh", "lab-ordered"),
         Spec(12, "sah", "lab-ordered"), Spec(13, "brute", "lab"), Spec(14, "brute", "lab"), Spec(15, "lbvh", "release"), Spec(16, "ploc", "release"),
         Spec(17, "sah", "release"), Spec(18, "upload", "lab"), Spec(19, "ploc", "lab"),
         Spec(20, "lbvh", "lab"))
_GENERATED = []
_COVERAGE = []


def sequence_of(index, n_steps=MAX_STEPS):
    """(Spec, [Step]) number `index` of SUITE.  The sequences are generated in order, each steered by the coverage of those before it (the brute-force ones
    stand beside it), once per process, and shared"""
    assert n_steps == MAX_STEPS
    if not _COVERAGE:
        _COVERAGE.append(Coverage())
    while len(_GENERATED) <= index:
        spec = SUITE[len(_GENERATED)]
        steps = sequence(spec.seed, spec.source, n_steps, _COVERAGE[0] if spec.source != "brute" else None)
        if spec.source != "brute":
            _COVERAGE[0].count(steps, spec.source)
        _GENERATED.append((spec, steps))
    return _GENERATED[index]


def suite():
    """([(Spec, [Step])] of SUITE, the coverage of its BVH sequences)"""
    sequence_of(len(SUITE) - 1)
    return list(_GENERATED), _COVERAGE[0]


# ---- steps that once differed from the model ---------------------------------------------------------------------------------------------------------------------

class Regression(NamedTuple):
    """step `step` of sequence(seed, source, step + 1), what it caught, and what that step must be: a predicate over (steps, index), held on the CPU by
    tests/test_scene_model_host.py, so that a change of the generator cannot quietly make the replay a test of something else"""
    seed: int
    source: str
    step: int
    what: str
    holds: object


def _sparse_refusal_with_a_device_list_after(kinds, source=None):
    def holds(steps, index):
        step, before = steps[index], steps[index - 1]
        return (index > 0 and step.kind == "refusal: an index twice in a sparse list" and step.on_device and before.kind in kinds
                and (source is None or (steps[0].form == "build" and steps[0].args[0] == source)))
    return holds


REGRESSION = (
    Regression(2, "ploc", 23, "a sparse update refused for an index that occurs twice, its list in device memory, directly after a rebuild: the library had made the "
               "inverse permutation for the validation kernels and kept its flag (have_inv_perm False -> True across a refusal); the flag now comes back",
               _sparse_refusal_with_a_device_list_after(REBUILDS, "ploc")),
    Regression(7, "sah", 12, "the same refusal directly after a guarded skin update that rebuilt, which discards the inverse permutation on a path of its own",
               _sparse_refusal_with_a_device_list_after(("skin-guarded-rebuild",))),
)
