"""Host-side mirror of the reference's `class RVPT` for the path this backend replaces.

Same names, argument meaning and frame-counter behaviour as src/rvpt/rvpt.{h,cpp}:
  add_material / add_triangle      rvpt.cpp:1041-1043
  initialize                        rvpt.cpp:56-94   (BVH build + permute, rvpt.cpp:83-86; resource creation)
  update                            rvpt.cpp:96-126  (accumulate-or-reset rule :102-111, uniform upload)
  draw                              rvpt.cpp:346-354 (record + submit of the compute pass)
  shutdown                          rvpt.cpp:407-442
Presentation (swapchain blit, ImGui, debug raster) is out of scope; read_frame() replaces the blit as the
way to get pixels out.  All GPU work goes through the C ABI (rvpt_amd.native); there is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import native, scene
from .camera import Camera


def wang_hash(v) -> np.ndarray:
    """util.glsl:25-33 on uint32 arrays (arithmetic modulo 2^32): the hash a pixel's index goes through before the frame number is added (util.glsl:35-36)"""
    v = np.array(v, dtype=np.uint32, copy=True)
    with np.errstate(over="ignore"):  # (a 0-d array multiplies as a scalar, which warns where arrays wrap silently)
        v = (v ^ np.uint32(61)) ^ (v >> np.uint32(16))
        v = v * np.uint32(9)
        v = v ^ (v >> np.uint32(4))
        v = v * np.uint32(0x27D4EB2D)
        v = v ^ (v >> np.uint32(15))
    return v


# The render modes a path query takes by name: eval_integrator's case labels 0 .. 9 (compute_pass.comp:76-95).  Hart, its default branch, is not part of the form.
PATH_MODE_NAMES = {"binary": 0, "color": 1, "depth": 2, "normal": 3, "utah": 4, "ao": 5, "appel": 6, "whitted": 7, "cook": 8, "kajiya": 9}


def path_mode(mode) -> int:
    """The render mode 0 .. 9 that `mode` — an int or a name of PATH_MODE_NAMES — stands for in RVPT.trace_paths; anything else raises native.NativeError."""
    if isinstance(mode, str):
        if mode not in PATH_MODE_NAMES:
            raise native.NativeError(native.ERR_INVALID, f"path query: unknown mode name {mode!r}; the names are {', '.join(PATH_MODE_NAMES)} (Hart is not part of the form)")
        return PATH_MODE_NAMES[mode]
    return native.format_ray_paths_mode(mode) - native.format_ray_paths_mode(0)


@dataclass
class RenderSettings:
    """rvpt.h:77-89 (defaults included: current_frame starts at 1 and is reset by the first update())."""
    max_bounces: int = 8
    aa: int = 1
    current_frame: int = 1
    camera_mode: int = 0
    top_left_render_mode: int = 9
    top_right_render_mode: int = 9
    bottom_left_render_mode: int = 9
    bottom_right_render_mode: int = 9
    split_ratio: tuple = field(default_factory=lambda: (0.5, 0.5))

    def pack(self) -> np.ndarray:
        """The 40-byte std140 block (compute_pass.comp:28-40)."""
        s = np.zeros(10, dtype=np.int32)
        s[0], s[1] = self.max_bounces, self.aa
        s.view(np.uint32)[2] = self.current_frame & 0xFFFFFFFF
        s[3] = self.camera_mode
        s[4:8] = (self.top_left_render_mode, self.top_right_render_mode, self.bottom_left_render_mode,
                  self.bottom_right_render_mode)
        s.view(np.float32)[8:10] = self.split_ratio
        return s

    def _reset_key(self):
        # PreviousFrameState::operator== (rvpt.cpp:21-29): aa and max_bounces are NOT part of it
        return ((float(np.float32(self.split_ratio[0])), float(np.float32(self.split_ratio[1]))), self.top_left_render_mode, self.top_right_render_mode,
                self.bottom_left_render_mode, self.bottom_right_render_mode, self.camera_mode)


def launch_sizes(frames: int, batch: int, in_flight: int = 3) -> list[int]:
    """How a run of `frames` accumulation frames with a still camera goes out: as few launches as `batch` allows, of near-equal size
    (20 frames at batch 8: 7 + 7 + 6; at batch 64: one launch of 20).  Measured on MI355X with the packet kernel
    (tools/archive/sweep_launch_shapes.sh, profiles/r03_launch_shapes.txt): on one GPU the shape of a 20-frame run does not matter (0.253-0.260 ms
    per frame for 20 / 10+10 / 7+7+6 / 5x4 / 4x5); on an eighth of the image ONE launch is best (0.0366 ms per frame against 0.0437 for
    7+7+6): a work-group of that kernel fills its CU's LDS share, launches in flight do not overlap, and every extra launch is an
    extra ramp and tail.  (Round 3 briefly forced at least `in_flight` launches — VERDICT r2 #2 — which cost the 8-rank case 19 %;
    the parameter is kept for callers and ignored.)  rvpt_host.cpp::launch_sizes is the same rule."""
    if frames <= 0:
        return []
    n = -(-frames // max(batch, 1))
    base, extra = divmod(frames, n)
    return [base + 1] * extra + [base] * (n - extra)


# the directions of RVPT.inside's three rays: none axis-aligned, none in a coordinate plane (they need not be unit)
INSIDE_DIRECTIONS = ((0.5377, 0.6197, 0.5717), (-0.6421, 0.3061, 0.7029), (0.2113, -0.8391, 0.5013))


def voxel_boxes(origin, cell, shape):
    """(lo, hi), float32[nx * ny * nz, 3] each: the closed cells of RVPT.voxelize's grid in C order of (i, j, k).  Along every axis cell i is
    [origin + i * cell, origin + (i + 1) * cell] in float32, one product and one sum, so neighbours share their face exactly; cell is a scalar or one edge
    per axis."""
    origin = np.broadcast_to(np.asarray(origin, dtype=np.float32), (3,))
    cell = np.broadcast_to(np.asarray(cell, dtype=np.float32), (3,))
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 0:
        raise ValueError(f"voxel_boxes: a shape (nx, ny, nz) is needed, got {shape}")
    index = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    return origin + index * cell, origin + (index + np.float32(1)) * cell


def crossing_rays(points):
    """(org[3n, 3], dir[3n, 3]) float32: the rays RVPT.inside asks, ray 3 i + j leaving point i along INSIDE_DIRECTIONS[j]"""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    return np.repeat(points, 3, axis=0), np.tile(np.asarray(INSIDE_DIRECTIONS, dtype=np.float32), (points.shape[0], 1))


def inside_from_crossings(front, back, rule="winding") -> np.ndarray:
    """RVPT.inside's vote over the counts of crossing_rays' 3 n rays: bool[n], true where at least two of a point's three rays say inside"""
    if rule not in ("winding", "parity"):
        raise ValueError(f"inside: rule must be 'winding' or 'parity', got {rule!r}")
    front, back = np.asarray(front, dtype=np.int64).reshape(-1, 3), np.asarray(back, dtype=np.int64).reshape(-1, 3)
    says = (back - front > 0) if rule == "winding" else ((front + back) % 2 == 1)
    return says.sum(axis=1) >= 2


def signed_distance_from(d2, prim, inside) -> np.ndarray:
    """RVPT.signed_distance from a point query's d2 and prim and RVPT.inside's answer: float32, +inf where the point query missed"""
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.asarray(d2, dtype=np.float32))
    d = np.where(np.asarray(inside, dtype=bool), -d, d).astype(np.float32)
    return np.where(np.asarray(prim) == native.NO_PRIM, np.float32(np.inf), d).astype(np.float32)


class RVPT:
    def __init__(self, width: int, height: int, device: int = 0, traversal: str = "brute", tile_rank: int = 0,
                 tile_world: int = 1, flags: int = 0, build: str = "host"):
        """build: who makes the tree of a BVH traversal — "host": rvpt_bvh_build (binned SAH, the reference's builder class) and a full upload; "device": the
        library builds an LBVH on the GPU from the triangles as they were added (Context.build_scene): two orders of magnitude quicker to build, slower to
        traverse; "device-ploc": the same with the PLOC tree (Context.build_scene(method="ploc"), scene.build_ploc); "device-sah": the same with
        rvpt_bvh_build's own binned-SAH tree made on the GPU (Context.build_scene(method="sah"), scene.build_sah)."""
        if traversal not in ("brute", "bvh", "bvh_ordered"):
            raise ValueError("traversal must be 'brute', 'bvh' (the reference's visiting order) or 'bvh_ordered'")
        if build not in ("host", "device", "device-ploc", "device-sah"):
            raise ValueError("build must be 'host', 'device', 'device-ploc' or 'device-sah'")
        self.build = build
        self.width, self.height = int(width), int(height)
        self.device, self.traversal = device, traversal
        self.tile_rank, self.tile_world = tile_rank, tile_world
        self._flags = flags | {"brute": native.TRAVERSAL_BRUTE, "bvh": native.TRAVERSAL_BVH,
                               "bvh_ordered": native.TRAVERSAL_BVH_ORDERED}[traversal]
        self.scene_camera = Camera(self.width / self.height)  # Window::get_aspect_ratio, window.cpp:89-92
        self.render_settings = RenderSettings()
        self.triangles: list[np.ndarray] = []
        self.materials: list[np.ndarray] = []
        self._bvh_nodes: np.ndarray | None = None
        self._nodes_stale = False  # update_triangles moved the geometry: bvh_nodes is refitted when it is next asked for
        self._stale_touched = None  # ... only the paths above these leaf-order positions (sparse updates since), None: the whole tree
        self._primitive_indices: np.ndarray | None = None
        self._sorted_triangles: np.ndarray | None = None
        self._built_from: np.ndarray | None = None  # build="device": the triangles the device built its tree from, until the host statement is asked for
        self._current_triangles: np.ndarray | None = None  # ... and the triangles the scene holds now, in the order they were added
        self._skin: np.ndarray | None = None  # bind_skin: the bound records, in the order the triangles were added
        self._rest_triangles: np.ndarray | None = None  # pose_parts: the rest pose, in the order they were added — the triangles as the last call of another form left them
        self._previous_key = None  # default-constructed PreviousFrameState never compares equal (empty camera data)
        self._ctx: native.Context | None = None
        self._n_triangles: int | None = None
        self._device_built = False

    # -- scene -------------------------------------------------------------------------------------------
    def add_material(self, material) -> None:
        self.materials.append(np.asarray(material, dtype=np.float32).reshape(12))

    def add_triangle(self, triangle) -> None:
        self.triangles.append(np.asarray(triangle, dtype=np.float32).reshape(1, 16))

    def add_triangles(self, triangles) -> None:
        self.triangles.append(np.asarray(triangles, dtype=np.float32).reshape(-1, 16))

    @property
    def bvh_nodes(self):
        """top_level_bvh (rvpt.h:175): the tree initialize() built; after update_triangles its refit (scene.refit_bvh), made when first asked for.  With
        build="device" / "device-ploc" / "device-sah" the tree lives on the GPU: what is returned is the same tree stated on the host (scene.build_lbvh / build_ploc /
        build_sah), made when first asked for."""
        self._host_statement()
        if self._nodes_stale:
            self._bvh_nodes = scene.refit_bvh(self._bvh_nodes, self.sorted_triangles, touched=self._stale_touched)
            self._nodes_stale, self._stale_touched = False, None
        return self._bvh_nodes

    @bvh_nodes.setter
    def bvh_nodes(self, nodes) -> None:
        self._bvh_nodes, self._nodes_stale, self._stale_touched = nodes, False, None

    def _host_statement(self) -> None:
        """build="device": bvh_nodes, primitive_indices and sorted_triangles of the device-built tree, from scene.build_lbvh (build_ploc for "device-ploc", build_sah for "device-sah") on the triangles it was built from"""
        if self._built_from is not None:
            built_from, self._built_from = self._built_from, None
            builder = {"device-ploc": scene.build_ploc, "device-sah": scene.build_sah}.get(self.build, scene.build_lbvh)
            self._bvh_nodes, self._primitive_indices = builder(built_from)[:2]
            self._sorted_triangles = self._current_triangles[self._primitive_indices]
            self._nodes_stale = self._current_triangles is not built_from  # moved since: the boxes are refitted when the nodes are asked for
            self._stale_touched = None

    @property
    def primitive_indices(self):
        self._host_statement()
        return self._primitive_indices

    @primitive_indices.setter
    def primitive_indices(self, idx) -> None:
        self._primitive_indices = idx

    @property
    def sorted_triangles(self):
        self._host_statement()
        return self._sorted_triangles

    @sorted_triangles.setter
    def sorted_triangles(self, tris) -> None:
        self._sorted_triangles = tris

    def update_triangles(self, triangles, rebuild_above=None, indices=None):
        """Moving geometry — what the per-frame triangle copy of rvpt.cpp:124 is for: `triangles` (float32[n, 16], in the order they were ADDED, same count) replace
        the scene's; the tree keeps its topology and is refitted on the device (Context.update_triangles), no rebuild.  The next update() restarts the accumulation.
        rebuild_above: Context.update_triangles' keyword — the guarded form: the refitted tree's SAH cost is reported (native.UpdateReport) and, past that factor of
        the cost of the tree as built, the device rebuilds by the builder of initialize().  A limit needs build="device*"; math.inf only reports.
        indices: the SPARSE form (Context.update_triangles' keyword) — `triangles` are k rows and replace the vertices of the triangles indices[j], numbered in the
        order they were ADDED; only the boxes above them are recomputed, on the device and in bvh_nodes.  Not together with rebuild_above."""
        if indices is not None:
            return self._update_sparse(triangles, rebuild_above, indices)
        tris = np.asarray(triangles, dtype=np.float32).reshape(-1, 16)
        if self._ctx is None or self._n_triangles is None:
            raise RuntimeError("update_triangles before initialize()")
        if tris.shape[0] != self._n_triangles:
            raise native.NativeError(native.ERR_INVALID, f"update_triangles: {tris.shape[0]} triangles given, the scene has {self._n_triangles}")
        if self._device_built:  # the device keeps the permutation: the caller's order goes down as it is
            report = self._ctx.update_triangles(tris, rebuild_above)
            self._current_triangles = tris.copy()
            self.triangles = [self._current_triangles]
            if report is not None and report.rebuilt:
                # the device holds a new tree and a new permutation: the host statement is that of a fresh build from these triangles, made when asked for
                self._built_from = self._current_triangles
                self._bvh_nodes = self._primitive_indices = self._sorted_triangles = None
                self._nodes_stale, self._stale_touched = False, None
            elif self._built_from is None:
                self._sorted_triangles = tris[self._primitive_indices]
                self._nodes_stale, self._stale_touched = True, None
        else:
            sorted_tris = tris[self.primitive_indices]  # leaf order (Bvh::permute_primitives)
            report = self._ctx.update_triangles(sorted_tris, rebuild_above)
            self.triangles = [tris.copy()]
            self.sorted_triangles = sorted_tris
            self._nodes_stale, self._stale_touched = self._bvh_nodes is not None, None
        self._previous_key = None  # a new scene: nothing accumulated so far belongs to it
        self._rest_triangles = None
        return report

    def _update_sparse(self, triangles, rebuild_above, indices) -> None:
        if self._ctx is None or self._n_triangles is None:
            raise RuntimeError("update_triangles before initialize()")
        if rebuild_above is not None:
            raise native.NativeError(native.ERR_INVALID, "update_triangles: indices (the sparse form) and rebuild_above (the guarded form) do not combine")
        tris = np.asarray(triangles, dtype=np.float32).reshape(-1, 16)
        idx = np.asarray(indices)
        if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)) or idx.shape[0] != tris.shape[0]:
            raise native.NativeError(native.ERR_INVALID, f"update_triangles: indices are a 1-D integer array with one entry per triangle given, got {idx.dtype} {idx.shape} for {tris.shape[0]}")
        if idx.size == 0:
            return None
        if int(idx.min()) < 0 or int(idx.max()) >= self._n_triangles:
            bad = int(np.flatnonzero((idx < 0) | (idx >= self._n_triangles))[0])
            raise native.NativeError(native.ERR_INVALID, f"update_triangles: indices[{bad}] = {int(idx[bad])} is outside the {self._n_triangles} triangles of the scene")
        idx = idx.astype(np.int64)
        if self._device_built:  # the device keeps the permutation: the caller's numbering goes down as it is
            self._ctx.update_triangles(tris, indices=idx)
        else:  # a host-built tree: added order -> leaf order through the inverse of primitive_indices
            inverse = np.empty(self._n_triangles, dtype=np.int64)
            inverse[np.asarray(self.primitive_indices, dtype=np.int64)] = np.arange(self._n_triangles)
            self._ctx.update_triangles(tris, indices=inverse[idx])
        # the mirror's host copies: only the vertex columns move, the material rows are the stored ones
        added = np.concatenate(self.triangles).copy() if self._current_triangles is None else self._current_triangles.copy()
        added[idx, :12] = tris[:, :12]
        self.triangles = [added]
        if self._device_built:
            self._current_triangles = added
        if self._built_from is None:  # there is a host statement to keep right
            inverse = np.empty(self._n_triangles, dtype=np.int64)
            inverse[np.asarray(self._primitive_indices, dtype=np.int64)] = np.arange(self._n_triangles)
            pos = inverse[idx]
            sorted_tris = self._sorted_triangles.copy()
            sorted_tris[pos, :12] = tris[:, :12]
            self._sorted_triangles = sorted_tris
            if self._bvh_nodes is not None:
                if not self._nodes_stale:
                    self._nodes_stale, self._stale_touched = True, pos
                elif self._stale_touched is not None:
                    self._stale_touched = np.concatenate([self._stale_touched, pos])
        self._previous_key = None  # a new scene: nothing accumulated so far belongs to it
        self._rest_triangles = None
        return None

    def pose_parts(self, moves, rebuild_above=None):
        """Rigid parts — the POSE UPDATE (Context.pose_parts; include/rvpt_hip.h): every move is (first, count, matrix) or a native.PART_MOVE_DTYPE record and
        names the triangles [first, first + count) in the order they were ADDED; the device poses them by the move's 3x4 matrix from the REST POSE — the
        triangles as the last initialize() or update_triangles left them; two poses of one part do not compose — and recomputes only the boxes above them, as in
        bvh_nodes.  scene.pose_parts is the statement.  The next update() restarts the accumulation, as after update_triangles.  After a host build a range of
        added triangles is scattered over the leaf order: it goes down as one record per run of consecutive positions, all with the part's matrix.
        rebuild_above: Context.pose_parts' keyword — the GUARDED form: the posed tree's SAH cost is reported (native.UpdateReport) and, past that factor of the cost
        of the tree as built, the device rebuilds by the builder of initialize() and carries its rest pose along; bvh_nodes, primitive_indices and sorted_triangles
        are then those of a fresh build of the posed triangles, made when asked for.  The rest copy kept here, in added order, stays.  A limit needs
        build="device*"; math.inf only reports."""
        if self._ctx is None or self._n_triangles is None:
            raise RuntimeError("pose_parts before initialize()")
        try:
            rec = scene.part_moves(moves)
        except (ValueError, TypeError) as e:
            raise native.NativeError(native.ERR_INVALID, f"pose_parts: {e}") from None
        if rec.shape[0] == 0:
            return None
        n = self._n_triangles
        current = np.concatenate(self.triangles) if self._current_triangles is None else self._current_triangles
        rest = current if self._rest_triangles is None else self._rest_triangles
        try:  # (ranges outside the scene and ranges that share a triangle: refused here in the added numbering, before anything is sent)
            if (rec["count"] == 0).any():
                raise ValueError(f"moves[{int(np.argmax(rec['count'] == 0))}] has a count of 0")
            posed = scene.pose_parts(rest, rec, current=current)
        except ValueError as e:
            raise native.NativeError(native.ERR_INVALID, f"pose_parts: {e}") from None
        idx = np.concatenate([np.arange(int(r["first"]), int(r["first"]) + int(r["count"]), dtype=np.int64) for r in rec])
        pos = None
        if self._built_from is None:  # (always so after a host build) added order -> leaf order through the inverse of primitive_indices
            inverse = np.empty(n, dtype=np.int64)
            inverse[np.asarray(self._primitive_indices, dtype=np.int64)] = np.arange(n)
            pos = inverse[idx]
        if self._device_built:  # the device keeps the permutation: the caller's numbering goes down as it is
            report = self._ctx.pose_parts(rec) if rebuild_above is None else self._ctx.pose_parts(rec, rebuild_above=rebuild_above)
        else:  # a host-built tree: added order -> runs of consecutive positions in leaf order
            runs = []
            for r in rec:
                p = np.sort(inverse[int(r["first"]):int(r["first"]) + int(r["count"])])
                starts = np.flatnonzero(np.concatenate([[True], np.diff(p) != 1]))
                ends = np.concatenate([starts[1:], [p.size]])
                run = np.zeros(starts.size, dtype=native.PART_MOVE_DTYPE)
                run["m"], run["first"], run["count"] = r["m"], p[starts], ends - starts
                runs.append(run)
            runs = np.concatenate(runs)
            report = self._ctx.pose_parts(runs) if rebuild_above is None else self._ctx.pose_parts(runs, rebuild_above=rebuild_above)
        self._rest_triangles = rest
        self.triangles = [posed]
        if self._device_built:
            self._current_triangles = posed
        if report is not None and report.rebuilt:
            # the device holds a new tree and a new permutation: the host statement is that of a fresh build from the posed triangles, made when asked for
            self._built_from = posed
            self._bvh_nodes = self._primitive_indices = self._sorted_triangles = None
            self._nodes_stale, self._stale_touched = False, None
        elif self._built_from is None:  # there is a host statement to keep right
            self._sorted_triangles = posed[np.asarray(self._primitive_indices, dtype=np.int64)]
            if self._bvh_nodes is not None:
                if not self._nodes_stale:
                    self._nodes_stale, self._stale_touched = True, pos
                elif self._stale_touched is not None:
                    self._stale_touched = np.concatenate([self._stale_touched, pos])
        self._previous_key = None  # a new scene: nothing accumulated so far belongs to it
        return report

    def bind_skin(self, skin, weights=None) -> None:
        """Skinning weights — the BIND (Context.bind_skin; include/rvpt_hip.h): four bone indices and four weights per vertex, what scene.vertex_skins takes (a
        native.VERTEX_SKIN_DTYPE array of three records per triangle, or indices[n, 3, 4] beside weights[n, 3, 4]), for the triangles in the order they were
        ADDED.  After a host build the records are reordered into leaf order with primitive_indices, the counterpart of pose_parts' runs; after a device build
        they go down as given.  Moves nothing and restarts nothing; a second bind replaces the first; initialize() drops the binding."""
        if self._ctx is None or self._n_triangles is None:
            raise RuntimeError("bind_skin before initialize()")
        try:
            rec = scene.vertex_skins(skin, weights)
        except (ValueError, TypeError) as e:
            raise native.NativeError(native.ERR_INVALID, f"bind_skin: {e}") from None
        if rec.shape[0] != 3 * self._n_triangles:
            raise native.NativeError(native.ERR_INVALID, f"bind_skin: {rec.shape[0]} records given, the scene has {self._n_triangles} triangles: three per triangle")
        if self._device_built:
            self._ctx.bind_skin(rec)
        else:
            self._ctx.bind_skin(np.ascontiguousarray(rec.reshape(-1, 3)[np.asarray(self.primitive_indices, dtype=np.int64)]).reshape(-1))
        self._skin = rec.copy()

    def skin(self, bones, rebuild_above=None):
        """Linear blend skinning — the SKIN UPDATE (Context.skin; include/rvpt_hip.h): `bones` (float32[k, 3, 4], [k, 12], or [k, 4, 4] with last rows 0 0 0 1) pose
        EVERY vertex from the REST POSE — pose_parts' rest pose: the triangles as the last initialize() or update_triangles left them; two skin updates do not
        compose — by the four weighted matrices bind_skin gave it; every box is refitted, on the device and in bvh_nodes.  scene.skin_triangles is the statement.
        The next update() restarts the accumulation, as after update_triangles.
        rebuild_above: Context.skin's keyword — the GUARDED form: the skinned tree's SAH cost is reported (native.UpdateReport) and, past that factor of the cost of
        the tree as built, the device rebuilds by the builder of initialize(), carries its rest pose along and keeps its binding; bvh_nodes, primitive_indices and
        sorted_triangles are then those of a fresh build of the skinned triangles, made when asked for.  The rest copy and the binding kept here, in added order,
        stay.  A limit needs build="device*"; math.inf only reports."""
        if self._ctx is None or self._n_triangles is None:
            raise RuntimeError("skin before initialize()")
        if self._skin is None:
            raise native.NativeError(native.ERR_INVALID, "skin: skin update before a bind (bind_skin)")
        current = np.concatenate(self.triangles) if self._current_triangles is None else self._current_triangles
        rest = current if self._rest_triangles is None else self._rest_triangles
        try:
            m = scene.bone_matrices(bones)
            skinned = scene.skin_triangles(rest, self._skin, m)
            skinned[:, 12:] = current[:, 12:]
        except (ValueError, TypeError) as e:
            raise native.NativeError(native.ERR_INVALID, f"skin: {e}") from None
        report = self._ctx.skin(m) if rebuild_above is None else self._ctx.skin(m, rebuild_above=rebuild_above)
        self._rest_triangles = rest
        self.triangles = [skinned]
        if self._device_built:
            self._current_triangles = skinned
        if report is not None and report.rebuilt:
            # the device holds a new tree and a new permutation: the host statement is that of a fresh build from the skinned triangles, made when asked for
            self._built_from = skinned
            self._bvh_nodes = self._primitive_indices = self._sorted_triangles = None
            self._nodes_stale, self._stale_touched = False, None
        elif self._built_from is None:  # there is a host statement to keep right: every box moves
            self._sorted_triangles = skinned[np.asarray(self._primitive_indices, dtype=np.int64)]
            self._nodes_stale, self._stale_touched = self._bvh_nodes is not None, None
        self._previous_key = None  # a new scene: nothing accumulated so far belongs to it
        return report

    # -- lifecycle -----------------------------------------------------------------------------------------
    def initialize(self) -> bool:
        tris = np.concatenate(self.triangles) if self.triangles else np.zeros((0, 16), np.float32)
        mats = np.stack(self.materials) if self.materials else np.zeros((0, 12), np.float32)
        self._n_triangles = tris.shape[0]
        self._rest_triangles = None
        self._skin = None
        self._device_built = self.build in ("device", "device-ploc", "device-sah") and self.traversal != "brute" and tris.shape[0] > 0
        self._ctx = native.Context(self.width, self.height, self.device, self.tile_rank, self.tile_world, self._flags)
        if self._device_built:
            self._ctx.build_scene(tris, mats, method={"device-ploc": "ploc", "device-sah": "sah"}.get(self.build, "lbvh"))
            self._built_from = self._current_triangles = tris
            return True
        if tris.shape[0]:
            # top_level_bvh = bvh_builder.build_bvh(triangles); sorted_triangles = permute_primitives (rvpt.cpp:83-86)
            self.bvh_nodes, self.primitive_indices = native.build_bvh(tris)
            self.sorted_triangles = tris[self.primitive_indices]
        else:
            self.bvh_nodes, self.primitive_indices, self.sorted_triangles = None, np.zeros(0, np.uint32), tris
        self._ctx.upload_scene(self.bvh_nodes if self.traversal != "brute" else None, self.sorted_triangles, mats)
        return True

    def update(self) -> bool:
        camera_data = self.scene_camera.get_data()
        rs = self.render_settings
        rs.camera_mode = self.scene_camera.mode
        # PreviousFrameState comparison (rvpt.cpp:21-29,102-111); camera_data is cached by the camera, so an
        # identity check short-cuts the byte comparison on the steady accumulate path
        # (compared by VALUE, float32 like the uniform block: a caller mutating rs.split_ratio in place must reset too)
        key = rs._reset_key()
        prev = self._previous_key
        same = prev is not None and prev[0] == key and (prev[1] is camera_data or prev[2] == camera_data.tobytes())
        if not same:
            rs.current_frame = 0
            self._previous_key = (key, camera_data, camera_data.tobytes())
        else:
            rs.current_frame += 1
        self._ctx.set_frame_fast(rs, camera_data)
        return True

    def draw(self) -> None:
        self._ctx.dispatch()

    def draw_frames(self, n_frames: int) -> None:
        """update(); draw_frames(n) == n x (update(); draw()) with nothing changed in between: the frames
        current_frame .. current_frame + n - 1 go out as one launch (rvpt_hip_dispatch_frames) and the frame
        counter moves on, so the next update() continues the accumulation."""
        self._ctx.dispatch_frames(n_frames)
        self.render_settings.current_frame += n_frames - 1

    def wait(self) -> None:
        self._ctx.wait()

    def read_frame(self, fmt: int = native.FORMAT_RGBA32F, out=None):
        """The frame as a numpy array; with out= (Context.read_into: a torch tensor on the context's device, where the frame then stays, or a numpy array) it is
        filled and returned instead."""
        if out is not None:
            return self._ctx.read_into(out, fmt)
        return self._ctx.read(fmt)

    def trace_rays(self, org, dir, tmax=float("inf"), any_hit=False, hits=None) -> np.ndarray:
        """Ray queries against the scene as it is now (Context.trace_rays; include/rvpt_hip.h: RAY QUERIES): closest — any_hit: first accepted — hit of every ray
        org + t dir, 0 < t < tmax.  Returns native.RAY_HIT_DTYPE records; prim numbers the triangles in the order they were ADDED (native.NO_PRIM: a miss), as
        update_triangles' indices do.  Needs initialize(), not update(): a query has no camera.  hits=k (1 .. native.RAY_MAX_HITS) returns records [n, k]: the
        k nearest hits of every ray, nearest first (K-NEAREST RAY QUERIES), prim numbered the same way."""
        if self._ctx is None:
            raise RuntimeError("trace_rays before initialize()")
        rec = self._ctx.trace_rays(org, dir, tmax, any_hit) if hits is None else self._ctx.trace_rays(org, dir, tmax, any_hit, hits=hits)
        if not self._device_built and rec.shape[0]:  # a host-built tree: the device numbers the leaf order it was given
            hit = rec["prim"] != native.NO_PRIM
            rec["prim"][hit] = np.asarray(self.primitive_indices, dtype=np.uint32)[rec["prim"][hit]]
        return rec

    def trace_paths(self, org, dir, seed=None, max_bounces=None, mode=None) -> np.ndarray:
        """Path queries against the scene as it is now (Context.trace_paths; include/rvpt_hip.h: PATH QUERIES): integrator_Kajiya's radiance along every ray
        org + t dir, as a frame's mode-9 pixel evaluates it for its camera ray.  seed (one RNG state per ray, or a scalar) defaults to what pixel i of a frame
        starts from before its two jitter values, wang_hash(i) + render_settings.current_frame; max_bounces to render_settings.max_bounces.  Returns
        native.RAY_PATH_DTYPE records: radiance, and the segments the path traced.  Needs initialize(), not update(): a query has no camera.
        mode — an int 0 .. 9 or a name of PATH_MODE_NAMES ("binary", "color", "depth", "normal", "utah", "ao", "appel", "whitted", "cook", "kajiya") — evaluates
        every record by that integrator instead (one mode per call; max_bounces is then the integrator's render_settings.max_bounces: the occlusion samples of
        "ao"); None is integrator_Kajiya, as before.  Hart is not part of the form: any other mode raises native.NativeError before any call."""
        mode = native.PATH_MODE_KAJIYA if mode is None else path_mode(mode)
        if self._ctx is None:
            raise RuntimeError("trace_paths before initialize()")
        n = np.asarray(org, dtype=np.float32).reshape(-1, 3).shape[0]
        if seed is None:
            seed = wang_hash(np.arange(n, dtype=np.uint32)) + np.uint32(self.render_settings.current_frame & 0xFFFFFFFF)
        if max_bounces is None:
            max_bounces = int(self.render_settings.max_bounces)
        return self._ctx.trace_paths(org, dir, seed, max_bounces, mode=mode)

    def closest_points(self, points, max_dist=float("inf"), k=None) -> np.ndarray:
        """Point queries against the scene as it is now (Context.closest_points; include/rvpt_hip.h: NEAREST POINTS): the nearest point of the mesh to every
        point of points[n, 3] within max_dist (a distance; the records carry it squared).  Returns native.POINT_HIT_DTYPE records: closest, d2 (the SQUARED
        distance), u, v, region, and prim numbering the triangles in the order they were ADDED (native.NO_PRIM: nothing within the bound), as trace_rays does.
        Over a host-built tree a tie between equal distances is broken on the stored number, before this renumbering.  Needs initialize(), not update().  k (1 .. native.POINT_MAX_NEAREST) returns records [n, k]: the
        k nearest triangles of every point, nearest first (K-NEAREST POINTS), prim of every filled slot numbered the same way."""
        if k is not None:
            native.FORMAT_NEAREST_POINTS_K(k)
        if self._ctx is None:
            raise RuntimeError("closest_points before initialize()")
        rec = self._ctx.closest_points(points, max_dist) if k is None else self._ctx.closest_points(points, max_dist, k=k)
        if not self._device_built and rec.shape[0]:  # a host-built tree: the device numbers the leaf order it was given
            hit = rec["prim"] != native.NO_PRIM
            rec["prim"][hit] = np.asarray(self.primitive_indices, dtype=np.uint32)[rec["prim"][hit]]
        return rec

    def count_crossings(self, org, dir, tmax=float("inf")) -> np.ndarray:
        """Crossing queries against the scene as it is now (Context.count_crossings; include/rvpt_hip.h: RAY CROSSINGS): for every ray org + t dir, 0 < t < tmax,
        how many triangles it passes facing it (front) and facing away (back), and the smallest and largest such t.  Returns native.RAY_CROSSINGS_DTYPE records;
        with no crossing front = back = 0, t_near = tmax, t_far = 0.  The answer names no triangle, so it is the same after every builder.  Needs initialize(),
        not update()."""
        if self._ctx is None:
            raise RuntimeError("count_crossings before initialize()")
        return self._ctx.count_crossings(org, dir, tmax)

    def box_overlaps(self, lo, hi, prim_from=0, k=1) -> np.ndarray:
        """Box queries against the scene as it is now (Context.box_overlaps; include/rvpt_hip.h: BOX OVERLAPS): how many triangles meet each closed box
        [lo[n, 3], hi[n, 3]] and the 4k - 1 smallest of their numbers.  Returns native.BOX_OVERLAP_DTYPE[n, k] (native.box_overlap_lists reads a group's count
        and list).  The listed numbers name the triangles in the order they were ADDED, as trace_rays does; over a host-built tree the library orders, cuts and
        compares with prim_from by the STORED number, before this renumbering, so there a list is not ascending and prim_from is a stored number — overlapping()
        pages for the caller and returns whole, sorted lists.  Needs initialize(), not update()."""
        if self._ctx is None:
            raise RuntimeError("box_overlaps before initialize()")
        rec = self._ctx.box_overlaps(lo, hi, prim_from, k)
        if not self._device_built and rec.shape[0]:  # a host-built tree: the device numbers the leaf order it was given
            quads = rec.view(np.uint32).reshape(rec.shape[0], int(k), 12)[:, :, 8:]
            hit = quads != native.NO_PRIM
            hit[:, 0, 0] = False  # (a group's first word is its count, not a number)
            quads[hit] = np.asarray(self.primitive_indices, dtype=np.uint32)[quads[hit]]
        return rec

    def sweep_spheres(self, org, dir, radius, tmax=float("inf"), contacts=False):
        """Sphere sweeps against the scene as it is now (Context.sweep_spheres; include/rvpt_hip.h: SPHERE SWEEPS): when and where the spheres of radius
        `radius` whose centres move along org[n, 3] + t dir[n, 3], t in [0, tmax], first touch the mesh.  Returns native.SPHERE_SWEEP_DTYPE records: t (in units
        of dir; 0 for a sphere that already overlaps), u, v, and prim numbering the triangles in the order they were ADDED (native.NO_PRIM: nothing touched, t =
        tmax), as trace_rays does.  Over a host-built tree a tie between equal times is broken on the stored number, before this renumbering.  contacts=True
        pipes the answer through surface_points and returns (records, native.SURFACE_POINT_DTYPE records): the contact point on the triangle, the stored unit
        normal and the material word of every hit, zeros and mat NO_PRIM beside a miss.  Needs initialize(), not update()."""
        if self._ctx is None:
            raise RuntimeError("sweep_spheres before initialize()")
        rec = self._ctx.sweep_spheres(org, dir, radius, tmax)
        if not self._device_built and rec.shape[0]:  # a host-built tree: the device numbers the leaf order it was given
            hit = rec["prim"] != native.NO_PRIM
            rec["prim"][hit] = np.asarray(self.primitive_indices, dtype=np.uint32)[rec["prim"][hit]]
        if not contacts:
            return rec
        return rec, self.surface_points(rec["prim"], rec["u"], rec["v"])

    def overlapping(self, lo, hi) -> list:
        """For every closed box [lo[n, 3], hi[n, 3]] the numbers of ALL triangles that meet it (BOX OVERLAPS: the set A with prim_from = 0), ascending, in the
        order the triangles were ADDED: a list of n uint32 arrays.  Pages with the longest groups (15 numbers a call) and prim_from = the last listed number + 1
        until every box has count numbers in hand; only the boxes that still have some to come are asked again.  Needs initialize(), not update()."""
        if self._ctx is None:
            raise RuntimeError("overlapping before initialize()")
        lo, hi = np.asarray(lo, dtype=np.float32).reshape(-1, 3), np.asarray(hi, dtype=np.float32).reshape(-1, 3)
        k = native.BOX_MAX_GROUP
        parts = [[] for _ in range(lo.shape[0])]
        ask, first = np.arange(lo.shape[0]), np.zeros(lo.shape[0], dtype=np.uint32)
        while ask.size:
            count, numbers = native.box_overlap_lists(self._ctx.box_overlaps(lo[ask], hi[ask], first, k), k)
            for row, box in enumerate(ask):
                parts[box].append(numbers[row][numbers[row] != native.NO_PRIM])
            more = count > numbers.shape[1]  # the list is full and there is more to come
            ask, first = ask[more], (numbers[more, -1] + np.uint32(1)).astype(np.uint32)
        out = [np.concatenate(p) if p else np.zeros(0, np.uint32) for p in parts]
        if not self._device_built and self._n_triangles:  # a host-built tree: stored numbers -> the order the triangles were added
            added = np.asarray(self.primitive_indices, dtype=np.uint32)
            out = [np.sort(added[o]) for o in out]
        return out

    def voxelize(self, origin, cell, shape) -> np.ndarray:
        """bool[nx, ny, nz]: the conservative SURFACE voxelisation of the mesh as it now stands — cell (i, j, k) of the grid voxel_boxes(origin, cell, shape)
        is set iff a box query counts at least one triangle meeting the closed cell, so a sliver between two cell centres still marks its cells (inside() only
        classifies points).  One box per cell, one call.  Needs initialize(), not update()."""
        if self._ctx is None:
            raise RuntimeError("voxelize before initialize()")
        lo, hi = voxel_boxes(origin, cell, shape)
        rec = self._ctx.box_overlaps(lo, hi)
        return (rec["count"][:, 0] > 0).reshape(tuple(int(s) for s in shape))

    def inside(self, points, rule="winding") -> np.ndarray:
        """bool[n]: whether each point of points[n, 3] lies inside the mesh as it is now.  Three rays leave every point along the three fixed directions
        INSIDE_DIRECTIONS = (0.5377, 0.6197, 0.5717), (-0.6421, 0.3061, 0.7029), (0.2113, -0.8391, 0.5013) — none axis-aligned, none in a coordinate plane —
        and each ray votes by its crossing counts (count_crossings, tmax = inf):
          rule="winding": inside iff back - front > 0.  Assumes a closed mesh whose normals point outward; nested and overlapping shells add up.
          rule="parity":  inside iff front + back is odd.  Assumes a closed mesh; the winding of its triangles does not matter.
        A point is inside iff at least two of its three rays say so.  The result is a VOTE, not a definition: a ray that meets an edge or a vertex exactly may
        count it twice or not at all, which is why there are three; on a mesh that is not closed the answer depends on the directions.  A point with a
        non-finite coordinate is outside.  Needs initialize(), not update()."""
        inside_from_crossings((), (), rule)  # (a wrong rule raises before any call)
        org, dirv = crossing_rays(points)
        rec = self.count_crossings(org, dirv)
        return inside_from_crossings(rec["front"], rec["back"], rule)

    def signed_distance(self, points) -> np.ndarray:
        """float32[n]: the distance from each point to the mesh as it is now — sqrt of closest_points' d2 — negative where inside(points) (the winding rule, with
        what it assumes) says inside; +inf where the point query misses (a non-finite point, the empty scene).  Needs initialize(), not update()."""
        points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        rec = self.closest_points(points)
        return signed_distance_from(rec["d2"], rec["prim"], self.inside(points))

    def read_triangles(self, out=None):
        """The mesh as it now stands on the device (Context.read_triangles; include/rvpt_hip.h: TRIANGLES): float32[n, 16], the stored bytes of every triangle
        after whatever update, pose or skin form ran last, rows in the order the triangles were ADDED.  After a device build out= (Context.read_triangles_into:
        a numpy array or a torch tensor on the context's device, where the rows then stay) is filled and returned instead; after a host build the device holds
        the leaf order, the rows go through primitive_indices here on the host, and out= must be a numpy array.  Needs initialize(), not update()."""
        if self._ctx is None:
            raise RuntimeError("read_triangles before initialize()")
        if self._device_built or self._n_triangles == 0:
            return self._ctx.read_triangles() if out is None else self._ctx.read_triangles_into(out)
        stored = self._ctx.read_triangles()
        if out is None:
            out = np.empty_like(stored)
        elif not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.ndim != 2 or out.shape[1] != 16 or out.shape[0] < stored.shape[0]:
            raise native.NativeError(native.ERR_INVALID, f"read_triangles: after a host build out= must be a numpy float32[n >= {stored.shape[0]}, 16] array")
        out[np.asarray(self.primitive_indices, dtype=np.int64)] = stored  # stored row s is added triangle primitive_indices[s]
        return out

    def surface_points(self, prim, u=None, v=None) -> np.ndarray:
        """Points on the mesh as it now stands (Context.surface_points; include/rvpt_hip.h: SURFACE POINTS) for triangles and pairs a query reported: prim[n]
        numbering the triangles in the order they were ADDED, as trace_rays and closest_points report it, with u[n], v[n] — or, alone, a native.RAY_HIT_DTYPE or
        native.POINT_HIT_DTYPE array, whose prim, u, v are taken.  Returns native.SURFACE_POINT_DTYPE records: point = (a + (b-a)*u) + (c-a)*v, the material
        word and the stored unit normal; prim comes back as given.  A miss (native.NO_PRIM) is an invalid record: zeros, mat NO_PRIM.  Needs initialize()."""
        if self._ctx is None:
            raise RuntimeError("surface_points before initialize()")
        if isinstance(prim, np.ndarray) and prim.dtype in (native.RAY_HIT_DTYPE, native.POINT_HIT_DTYPE):
            if u is not None or v is not None:
                raise native.NativeError(native.ERR_INVALID, "surface_points: query records carry their own u and v")
            prim, u, v = prim["prim"], prim["u"], prim["v"]
        elif u is None or v is None:
            raise native.NativeError(native.ERR_INVALID, "surface_points: prim, u and v are needed, or an array of RAY_HIT_DTYPE / POINT_HIT_DTYPE records")
        prim = np.asarray(prim)
        if self._device_built or prim.size == 0 or prim.dtype.kind not in "iu":  # (Context.surface_points refuses what is no integer)
            return self._ctx.surface_points(prim, u, v)
        # a host-built tree: added order -> leaf order through the inverse of primitive_indices; what is outside the scene stays outside
        given = prim.reshape(-1).astype(np.int64)
        inverse = np.empty(self._n_triangles, dtype=np.int64)
        inverse[np.asarray(self.primitive_indices, dtype=np.int64)] = np.arange(self._n_triangles)
        inside = (given >= 0) & (given < self._n_triangles)
        stored = np.where(inside, inverse[np.where(inside, given, 0)] if self._n_triangles else 0, native.NO_PRIM)
        rec = self._ctx.surface_points(stored.astype(np.uint32), u, v)
        rec["prim"] = given.astype(np.uint32)
        return rec

    def pick(self, x: int, y: int, hits=None):
        """What is under pixel (x, y) of the current camera: (prim, t) of the closest hit along the pixel-centre ray, or None.  The ray is made HERE, on the host, from
        scene_camera.get_data() (camera.glsl:29-51 in double, rounded to float32 once) — not by the frame kernel's float32 arithmetic: t agrees with a frame's to
        rounding, not to the bit.  Pinhole camera only.  hits=k (1 .. native.RAY_MAX_HITS) is the x-ray pick: the list of (prim, t) of the k nearest surfaces
        along that ray, nearest first, shorter where the ray meets fewer and empty on a miss."""
        if hits is not None:
            native.FORMAT_RAY_HITS_NEAREST(hits)
            if self._ctx is None:
                raise RuntimeError("pick before initialize()")
        if self.scene_camera.mode != 0:
            raise ValueError("pick: only the pinhole camera (mode 0) has a pixel-centre ray made here")
        if not (0 <= int(x) < self.width and 0 <= int(y) < self.height):
            raise ValueError(f"pick: pixel ({x}, {y}) is outside the {self.width} x {self.height} frame")
        cam = np.asarray(self.scene_camera.get_data(), dtype=np.float64)
        m = cam[:16].reshape(4, 4).T  # column-major camera-to-world
        cx, cy = (int(x) + 0.5) / self.width, 1.0 - (int(y) + 0.5) / self.height  # compute_pass.comp:151-156
        d = m[:3, :3] @ np.array([cam[16] * (2.0 * cx - 1.0), 2.0 * cy - 1.0, 1.0 / np.tan(0.5 * cam[17])])
        d /= np.linalg.norm(d)
        if hits is not None:
            return [(int(r["prim"]), float(r["t"])) for r in self.trace_rays(m[:3, 3], d, hits=hits)[0] if r["prim"] != native.NO_PRIM]
        rec = self.trace_rays(m[:3, 3], d)[0]
        return None if rec["prim"] == native.NO_PRIM else (int(rec["prim"]), float(rec["t"]))

    def shutdown(self) -> None:
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    @property
    def context(self) -> native.Context:
        return self._ctx
