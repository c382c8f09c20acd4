"""ctypes bindings of the C ABI (include/rvpt_hip.h).

There is no fallback: if librvpt_hip.so is missing or a call fails, NativeError is raised.
"""
from __future__ import annotations

import ctypes as C
import math
import re
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np

_PKG = Path(__file__).resolve().parent
_LIB = None
_LAB = None

# include/rvpt_hip.h constants
ABI_VERSION = 8
BUILD_LAB, BUILD_DEBUG_CHECKS = 0x1, 0x2  # rvpt_hip_build_flags
MAX_FRAMES_PER_DISPATCH = 64
TRAVERSAL_BRUTE, TRAVERSAL_BVH, TRAVERSAL_BVH_ORDERED = 0x0, 0x1, 0x2
COUNT_SEGMENTS, KERNEL_SIMPLE, TIMING, ACCUM_UNORM8 = 0x4, 0x8, 0x10, 0x20
BVH_PER_LANE = 0x400  # BVH contexts: no camera packets, every segment walks the tree per lane (rounds 1-3's kernel)
BRUTE_MIXED_PACKETS = 0x200  # brute-force contexts: round 2's mixed-packet frame kernel instead of the packet kernel (rvpt_packets.hip)
FORMAT_RGBA32F, FORMAT_RGBA8_UNORM = 0, 1
FORMAT_RAY_HITS = 2  # RVPT_HIP_FORMAT_RAY_HITS: rvpt_hip_read answers ray queries, `dst` holds RAY_HIT_DTYPE records (Context.trace_rays)
RAY_ANY_HIT = 0x1  # RVPT_HIP_RAY_ANY_HIT: a record's flag — stop at the first accepted triangle
RAY_MAX_HITS = 8  # RVPT_HIP_RAY_MAX_HITS: the largest k of a k-nearest ray query

NO_PRIM = 0xFFFFFFFF  # a record's prim after a miss
# rvpt_ray_hit (48 B): org, tmax, dir, flags come in, t, prim, u, v go out
RAY_HIT_DTYPE = np.dtype([("org", "<f4", (3,)), ("tmax", "<f4"), ("dir", "<f4", (3,)), ("flags", "<u4"), ("t", "<f4"), ("prim", "<u4"), ("u", "<f4"), ("v", "<f4")])
FORMAT_RAY_CROSSINGS = 8  # RVPT_HIP_FORMAT_RAY_CROSSINGS: rvpt_hip_read answers crossing queries, `dst` holds RAY_CROSSINGS_DTYPE records (Context.count_crossings)
# rvpt_ray_crossings (48 B): org, tmax, dir, flags come in as for a ray query (flags is ignored), front, back, t_near, t_far go out
RAY_CROSSINGS_DTYPE = np.dtype([("org", "<f4", (3,)), ("tmax", "<f4"), ("dir", "<f4", (3,)), ("flags", "<u4"), ("front", "<u4"), ("back", "<u4"), ("t_near", "<f4"), ("t_far", "<f4")])
FORMAT_RAY_PATHS = 3  # RVPT_HIP_FORMAT_RAY_PATHS: rvpt_hip_read answers path queries, `dst` holds RAY_PATH_DTYPE records (Context.trace_paths)
PATH_MODE_KAJIYA = 9  # the render mode of integrator_Kajiya: format_ray_paths_mode(9) is FORMAT_RAY_PATHS' own kernels and bytes


def format_ray_paths_mode(mode) -> int:
    """RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode): the format of a path query whose records are evaluated by the integrator of render mode 0 .. 9
    (compute_pass.comp:76-95: binary, color, depth, normal, Utah, ambient occlusion, Appel, Whitted, Cook, Kajiya).  Any other mode — Hart is 10 — raises."""
    if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)):
        raise NativeError(ERR_INVALID, f"path query: mode {mode!r} is not an integer; render modes 0 .. 9 are built (Hart is not part of the form)")
    if not 0 <= int(mode) <= PATH_MODE_KAJIYA:
        raise NativeError(ERR_INVALID, f"path query: mode {int(mode)} is outside 0 .. 9; integrator_Hart and the modes that default to it are not part of the form")
    return 16 + int(mode)


def FORMAT_RAY_HITS_NEAREST(k) -> int:
    """RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k), formats 33 .. 40: `dst` holds groups of k RAY_HIT_DTYPE records, the ray in the first, its k nearest hits out
    (Context.trace_rays(..., hits=k)).  A k that is no int in 1 .. RAY_MAX_HITS raises before any call."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= RAY_MAX_HITS:
        raise NativeError(ERR_INVALID, f"hits must be an int in 1 .. {RAY_MAX_HITS}, got {k!r}")
    return 32 + int(k)
PATH_MAX_BOUNCES = 1024  # RVPT_HIP_PATH_MAX_BOUNCES: a record with a larger bounce budget, or with none, is invalid (radiance 0, segments 0)
# rvpt_ray_path (48 B): org, seed, dir, max_bounces come in, radiance and segments go out
RAY_PATH_DTYPE = np.dtype([("org", "<f4", (3,)), ("seed", "<u4"), ("dir", "<f4", (3,)), ("max_bounces", "<u4"), ("radiance", "<f4", (3,)), ("segments", "<u4")])
FORMAT_NEAREST_POINTS = 4  # RVPT_HIP_FORMAT_NEAREST_POINTS: rvpt_hip_read answers point queries, `dst` holds POINT_HIT_DTYPE records (Context.closest_points)
# rvpt_point_hit: 48 bytes, three float4 — a point and a SQUARED bound in; the nearest point of the mesh, its squared distance, the triangle, u, v and the region out
POINT_HIT_DTYPE = np.dtype([("point", "<f4", (3,)), ("max_d2", "<f4"), ("closest", "<f4", (3,)), ("d2", "<f4"), ("prim", "<u4"), ("u", "<f4"), ("v", "<f4"), ("region", "<u4")])
POINT_MAX_NEAREST = 8  # RVPT_HIP_POINT_MAX_NEAREST: the largest k of a k-nearest point query


def FORMAT_NEAREST_POINTS_K(k) -> int:
    """RVPT_HIP_FORMAT_NEAREST_POINTS_K(k), formats 49 .. 56: `dst` holds groups of k POINT_HIT_DTYPE records, the point in the first, its k nearest triangles
    out (Context.closest_points(..., k=k)).  A k that is no int in 1 .. POINT_MAX_NEAREST raises before any call."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= POINT_MAX_NEAREST:
        raise NativeError(ERR_INVALID, f"k must be an int in 1 .. {POINT_MAX_NEAREST}, got {k!r}")
    return 48 + int(k)


FORMAT_BOX_OVERLAPS = 9  # RVPT_HIP_FORMAT_BOX_OVERLAPS: rvpt_hip_read answers box queries, `dst` holds BOX_OVERLAP_DTYPE records (Context.box_overlaps)
# rvpt_box_overlap: 48 bytes, three float4 — a closed box [lo, hi] and the first number that takes part in; the count of the triangles that meet it and the smallest of their numbers out
BOX_OVERLAP_DTYPE = np.dtype([("lo", "<f4", (3,)), ("prim_from", "<u4"), ("hi", "<f4", (3,)), ("flags", "<u4"), ("count", "<u4"), ("prim", "<u4", (3,))])
BOX_MAX_GROUP = 4  # RVPT_HIP_BOX_MAX_GROUP: the largest k of a box query's groups, which list 4k - 1 numbers


FORMAT_SPHERE_SWEEPS = 10  # RVPT_HIP_FORMAT_SPHERE_SWEEPS: rvpt_hip_read answers sphere sweeps, `dst` holds SPHERE_SWEEP_DTYPE records (Context.sweep_spheres)
# rvpt_sphere_sweep (== scene.SPHERE_SWEEP_DTYPE): the out quad is laid out as RAY_HIT_DTYPE's
SPHERE_SWEEP_DTYPE = np.dtype([("org", "<f4", (3,)), ("radius", "<f4"), ("dir", "<f4", (3,)), ("tmax", "<f4"), ("t", "<f4"), ("prim", "<u4"), ("u", "<f4"), ("v", "<f4")])


def FORMAT_BOX_OVERLAPS_K(k) -> int:
    """RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k), formats 65 .. 68: `dst` holds groups of k BOX_OVERLAP_DTYPE records, the box in the first, count and 4k - 1 numbers
    out (Context.box_overlaps(..., k=k)); k = 1 is FORMAT_BOX_OVERLAPS' own kernels and bytes.  A k that is no int in 1 .. BOX_MAX_GROUP raises before any call."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= BOX_MAX_GROUP:
        raise NativeError(ERR_INVALID, f"k must be an int in 1 .. {BOX_MAX_GROUP}, got {k!r}")
    return 64 + int(k)


def box_overlap_lists(records, k=1):
    """(count[n], numbers[n, 4k - 1]) of answered box records (BOX_OVERLAP_DTYPE, n groups of k, flat or [n, k]): the lists of a group side by side"""
    g = np.ascontiguousarray(records).reshape(-1, int(k))
    quads = g.view(np.uint32).reshape(g.shape[0], int(k), 12)[:, :, 8:].reshape(g.shape[0], 4 * int(k))
    return quads[:, 0].copy(), quads[:, 1:].copy()


FORMAT_TRIANGLES = 5  # RVPT_HIP_FORMAT_TRIANGLES: rvpt_hip_read returns the stored rvpt_triangle rows in update order (Context.read_triangles)
FORMAT_SURFACE_POINTS = 6  # RVPT_HIP_FORMAT_SURFACE_POINTS: rvpt_hip_read answers surface records, `dst` holds SURFACE_POINT_DTYPE records (Context.surface_points)
# rvpt_surface_point: 48 bytes, three float4 — prim, u, v as a query reported them (and a reserved word) in; the point of the stored mesh, its material word, its normal out
SURFACE_POINT_DTYPE = np.dtype([("prim", "<u4"), ("u", "<f4"), ("v", "<f4"), ("flags", "<u4"), ("point", "<f4", (3,)), ("mat", "<u4"), ("normal", "<f4", (3,)), ("reserved", "<u4")])
CULL_ROW_BOXES = 0x100  # Context.cull_info: the launch rode with the row boxes (rvpt_abi.hip: kCullRowBoxes)
CULL_ROW_RULE_TIGHT = 0x400  # Context.cull_info: ... made by the tight rule (rvpt_abi.hip: kCullRowRuleTight; rvpt_vis.h: kRowRuleTight)
CULL_ROW_CAPS = 0x800  # Context.cull_info: ... and with finite row caps, which let uniform rounds skip their walk (rvpt_abi.hip: kCullRowCaps; rvpt_vis.h: the row caps)
CULL_SKY_LIST = 0x80 # Context.cull_info: the launch took the listed path (rvpt_abi.hip: kCullSkyList)
CULL_FRAME_RUNS = 0x200  # Context.cull_info: ... in frame-run order, the camera set-up of a block made once per run (rvpt_abi.hip: kCullFrameRuns)
TILE = 16
TILE_SHIFT = 3  # RVPT_HIP_TILE_SHIFT: every row of the tile grid is rotated by this many more tiles than the one above (tile ownership)
NODES_BUILD = C.c_size_t(-1).value  # RVPT_HIP_NODES_BUILD: upload_scene's node count for the build form (Context.build_scene)
NODES_BUILD_SAH = C.c_size_t(-3).value  # RVPT_HIP_NODES_BUILD_SAH: the build form with rvpt_bvh_build's binned-SAH tree (Context.build_scene(method="sah"))
NODES_UPDATE_SPARSE = C.c_size_t(-4).value  # RVPT_HIP_NODES_UPDATE_SPARSE: the sparse update (Context.update_triangles(indices=)): `nodes` then carries the indices
NODES_UPDATE_POSE = C.c_size_t(-5).value  # RVPT_HIP_NODES_UPDATE_POSE: the pose update (Context.pose_parts): `nodes` then carries PART_MOVE_DTYPE records, no triangles
# rvpt_part_move (64 B): a 3x4 matrix, row major, for the triangles [first, first + count); two reserved words, 0
PART_MOVE_DTYPE = np.dtype([("m", "<f4", (12,)), ("first", "<u4"), ("count", "<u4"), ("reserved", "<u4", (2,))])
NODES_BIND_SKIN = C.c_size_t(-6).value  # RVPT_HIP_NODES_BIND_SKIN: the bind (Context.bind_skin): `nodes` then carries three VERTEX_SKIN_DTYPE records per triangle, no triangles
NODES_UPDATE_SKIN = C.c_size_t(-7).value  # RVPT_HIP_NODES_UPDATE_SKIN: the skin update (Context.skin): `nodes` then carries BONE_DTYPE matrices, no triangles
SKIN_MAX_BONES = 1024  # RVPT_HIP_SKIN_MAX_BONES
# rvpt_vertex_skin (32 B): the four bone indices and the four weights of one vertex;  rvpt_bone (48 B): a 3x4 matrix, row major
VERTEX_SKIN_DTYPE = np.dtype([("bone", "<u4", (4,)), ("weight", "<f4", (4,))])
BONE_DTYPE = np.dtype([("m", "<f4", (12,))])
NODES_UPDATE_GUARDED_BASE = 0x10000  # RVPT_HIP_NODES_UPDATE_GUARDED(permille) = (size_t)0 - (0x10000 + permille): the guarded update (Context.update_triangles(rebuild_above=))
NODES_UPDATE_POSE_GUARDED_BASE = 0x200000  # RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) = (size_t)0 - (0x200000 + permille): the guarded pose update (Context.pose_parts(rebuild_above=))
NODES_UPDATE_SKIN_GUARDED_BASE = 0x300000  # RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille) = (size_t)0 - (0x300000 + permille): the guarded skin update (Context.skin(rebuild_above=))
NODES_BUILD_PLOC = C.c_size_t(-2).value  # RVPT_HIP_NODES_BUILD_PLOC: the build form with a PLOC tree (Context.build_scene(method="ploc"))
ERR_INVALID, ERR_HIP, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_SIZE, ERR_COMM = -1, -2, -3, -4, -5, -6

# the C ABI of include/rvpt_hip.h: what librvpt_hip.so exports, all of it and nothing else (tests/test_abi_exports.py)
EXPORTS = [
    "rvpt_hip_abi_version", "rvpt_hip_build_flags", "rvpt_hip_device_count", "rvpt_hip_create", "rvpt_hip_destroy",
    "rvpt_hip_upload_scene", "rvpt_hip_set_frame", "rvpt_hip_dispatch", "rvpt_hip_dispatch_frames", "rvpt_hip_wait", "rvpt_hip_wait_for", "rvpt_hip_query",
    "rvpt_hip_read", "rvpt_hip_tile_buffer", "rvpt_hip_untile", "rvpt_hip_write_accum", "rvpt_hip_get_timing",
    "rvpt_hip_reset_timing", "rvpt_hip_get_stats", "rvpt_hip_get_launch_info", "rvpt_hip_get_cull_info", "rvpt_hip_last_error", "rvpt_bvh_build",
    "rvpt_hip_comm_unique_id", "rvpt_hip_comm_init", "rvpt_hip_comm_init_all", "rvpt_hip_comm_info", "rvpt_hip_gather", "rvpt_hip_comm_barrier", "rvpt_hip_comm_destroy",
]
# ... and what the laboratory build librvpt_hip_debug.so adds (include/rvpt_hip_lab.h)
LAB_EXPORTS = [
    "rvpt_hip_selftest_div", "rvpt_hip_selftest_rcp", "rvpt_hip_selftest_pretest", "rvpt_hip_selftest_camera_rects", "rvpt_hip_selftest_bounce_cull",
    "rvpt_hip_selftest_fast_div", "rvpt_camera_rects", "rvpt_bounce_rows", "rvpt_bounce_leaf_boxes", "rvpt_bvh_wide_form", "rvpt_claim_order",
    "rvpt_hip_selftest_scene_state",
]


def nodes_update_guarded(permille: int) -> int:
    """RVPT_HIP_NODES_UPDATE_GUARDED(permille) of include/rvpt_hip.h as the size_t the call takes"""
    return C.c_size_t(-(NODES_UPDATE_GUARDED_BASE + int(permille))).value


def nodes_update_pose_guarded(permille: int) -> int:
    """RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) of include/rvpt_hip.h as the size_t the call takes"""
    return C.c_size_t(-(NODES_UPDATE_POSE_GUARDED_BASE + int(permille))).value


def nodes_update_skin_guarded(permille: int) -> int:
    """RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille) of include/rvpt_hip.h as the size_t the call takes"""
    return C.c_size_t(-(NODES_UPDATE_SKIN_GUARDED_BASE + int(permille))).value


def _guard_permille(rebuild_above, who: str) -> int:
    """rebuild_above of the guarded forms as the permille their counts carry: a float >= 1 rounded to thousandths, math.inf is 0 (report only)"""
    limit = float(rebuild_above)
    permille = 0 if limit == math.inf else int(round(min(limit, 1e6) * 1000.0)) if limit == limit and limit > 0 else -1
    if permille != 0 and not 1000 <= permille <= 65535:
        raise NativeError(ERR_INVALID, f"{who}: rebuild_above is a factor in [1, 65.535] or math.inf (report only), got {rebuild_above!r}")
    return permille


class UpdateReport(NamedTuple):
    """What a guarded update, a guarded pose update or a guarded skin update reports: the refitted tree's SAH cost, the cost of the tree as it was last built or uploaded, cost / base_cost (0.0 when the base is
    0), whether the library rebuilt, and then the builder's name ("lbvh", "ploc", "sah"; None after a refit)."""
    cost: float
    base_cost: float
    ratio: float
    rebuilt: bool
    tree: Optional[str]


_GUARD_SENTENCE = re.compile(r"guarded (?:pose |skin )?update: cost (\S+), base cost (\S+), limit (\d+) permille: (?:refitted|rebuilt \((lbvh|ploc|sah)\), new base cost (\S+))\Z")


def parse_update_report(sentence: str) -> UpdateReport:
    """The one sentence rvpt_hip_last_error holds after a guarded update, a guarded pose update or a guarded skin update (include/rvpt_hip.h fixes the wordings)"""
    m = _GUARD_SENTENCE.match(sentence)
    if m is None:
        raise NativeError(ERR_INVALID, f"update_triangles: not a guarded update's report: {sentence!r}")
    cost, base = float(m.group(1)), float(m.group(2))
    return UpdateReport(cost, base, cost / base if base > 0.0 else 0.0, m.group(4) is not None, m.group(4))


def _report_of(ctx, rebuild_above):
    """what a guarded form returns: None for the plain call and on a brute-force context, which holds no tree; the parsed sentence otherwise"""
    if rebuild_above is None or (ctx.flags & (TRAVERSAL_BVH | TRAVERSAL_BVH_ORDERED)) == 0:
        return None
    return parse_update_report((ctx._L.rvpt_hip_last_error(ctx._h) or b"").decode())


class SceneStateInfo(C.Structure):
    """rvpt_hip_scene_state_info (include/rvpt_hip_lab.h)"""
    _fields_ = [("n_tris", C.c_uint64), ("n_nodes", C.c_uint64), ("n_wide", C.c_uint64),
                ("bvh_head_shift", C.c_uint32), ("wide_stack_levels", C.c_uint32), ("bvh_height", C.c_uint32), ("built_by", C.c_uint32),
                ("have_perm", C.c_uint32), ("have_sparse_maps", C.c_uint32), ("have_inv_perm", C.c_uint32), ("have_cost", C.c_uint32),
                ("base_cost", C.c_double)]


class NativeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"rvpt_hip error {code}: {message}")
        self.code = code


def lib_path(lab: bool = False) -> Path:
    """In-tree library: librvpt_hip.so, or the laboratory build librvpt_hip_debug.so (include/rvpt_hip_lab.h).  RVPT_HIP_LIB overrides the release path
    (kernel experiments: tools/archive/exp_variants.py), RVPT_HIP_LAB_LIB the laboratory one."""
    import os
    override = os.environ.get("RVPT_HIP_LAB_LIB" if lab else "RVPT_HIP_LIB")
    return Path(override) if override else _PKG / ("librvpt_hip_debug.so" if lab else "librvpt_hip.so")


def _bind(L, lab: bool):
    vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    L.rvpt_hip_abi_version.restype = i32
    L.rvpt_hip_build_flags.restype = u32
    L.rvpt_hip_device_count.argtypes = [C.POINTER(i32)]
    L.rvpt_hip_create.argtypes = [C.POINTER(vp), i32, u32, u32, u32, u32, u32]
    L.rvpt_hip_destroy.argtypes = [vp]
    L.rvpt_hip_destroy.restype = None
    L.rvpt_hip_upload_scene.argtypes = [vp, vp, sz, vp, sz, vp, sz]
    L.rvpt_hip_set_frame.argtypes = [vp, vp, vp]
    L.rvpt_hip_dispatch.argtypes = [vp]
    L.rvpt_hip_dispatch_frames.argtypes = [vp, C.c_uint32]
    L.rvpt_hip_wait_for.argtypes = [vp, C.c_uint64]
    L.rvpt_hip_wait.argtypes = [vp]
    L.rvpt_hip_query.argtypes = [vp]
    L.rvpt_hip_read.argtypes = [vp, i32, vp, sz]
    L.rvpt_hip_tile_buffer.argtypes = [vp, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]
    L.rvpt_hip_untile.argtypes = [vp, vp, sz, u32, vp]
    L.rvpt_hip_write_accum.argtypes = [vp, vp, sz]
    L.rvpt_hip_get_timing.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.rvpt_hip_reset_timing.argtypes = [vp]
    L.rvpt_hip_get_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rvpt_hip_get_launch_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.rvpt_hip_get_cull_info.argtypes = [vp, C.POINTER(u32)]
    L.rvpt_hip_last_error.argtypes = [vp]
    L.rvpt_hip_last_error.restype = C.c_char_p
    L.rvpt_bvh_build.argtypes = [vp, sz, vp, C.POINTER(sz), vp]
    L.rvpt_hip_comm_unique_id.argtypes = [vp, sz]
    L.rvpt_hip_comm_init.argtypes = [vp, vp, sz]
    L.rvpt_hip_comm_init_all.argtypes = [C.POINTER(vp), i32]
    L.rvpt_hip_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.rvpt_hip_gather.argtypes = [vp, vp]
    L.rvpt_hip_comm_barrier.argtypes = [vp]
    L.rvpt_hip_comm_destroy.argtypes = [vp]
    names = list(EXPORTS)
    if lab:
        L.rvpt_bvh_wide_form.argtypes = [vp, sz, C.c_uint32, vp, sz, C.POINTER(sz), C.POINTER(C.c_uint32)]
        L.rvpt_hip_selftest_div.argtypes = [i32, vp, vp, vp, sz]
        L.rvpt_hip_selftest_rcp.argtypes = [i32, vp]
        L.rvpt_hip_selftest_pretest.argtypes = [i32, vp, vp, vp, vp, sz]
        L.rvpt_camera_rects.argtypes = [vp, sz, vp, u32, u32, vp]
        L.rvpt_bounce_rows.argtypes = [vp, vp, sz, vp, C.POINTER(C.c_double)]
        L.rvpt_bounce_leaf_boxes.argtypes = [vp, sz, vp, C.POINTER(u32), vp]
        L.rvpt_claim_order.argtypes = [u32, u32, vp, vp]
        L.rvpt_hip_selftest_camera_rects.argtypes = [vp, u32, vp, vp, vp]
        L.rvpt_hip_selftest_bounce_cull.argtypes = [vp, u32, vp]
        L.rvpt_hip_selftest_fast_div.argtypes = [u32, vp, vp, sz]
        L.rvpt_hip_selftest_scene_state.argtypes = [vp, C.POINTER(SceneStateInfo), u32, vp, sz, C.POINTER(sz)]
        names += LAB_EXPORTS
    for name in names:
        if name not in ("rvpt_hip_destroy", "rvpt_hip_last_error", "rvpt_hip_build_flags"):
            getattr(L, name).restype = i32
    if L.rvpt_hip_abi_version() != ABI_VERSION:
        raise NativeError(ERR_INVALID, f"ABI version {L.rvpt_hip_abi_version()} != {ABI_VERSION}")
    if lab and not (L.rvpt_hip_build_flags() & BUILD_LAB):
        raise NativeError(ERR_INVALID, "the laboratory library was not built with -DRVPT_HIP_LAB=1 (rvpt_amd.build.build_native_debug)")
    return L


def _open(lab: bool) -> C.CDLL:
    # torch bundles its own ROCm runtime (libamdhip64.so.7 + HSA) and must be the first to load it: if
    # the system copy of the same SONAME gets in first (through this library's DT_NEEDED), torch ends up
    # on a mixed runtime that sees no device.  torch is only plumbing here, but load order matters.
    import torch  # noqa: F401
    path = lib_path(lab)
    if not path.exists():
        raise NativeError(ERR_HIP, f"{path} not found — run `python -m rvpt_amd.build` (hipcc, gfx950); "
                                   "there is no CPU fallback")
    return _bind(C.CDLL(str(path)), lab)


def load() -> C.CDLL:
    """Load librvpt_hip.so (built in-tree by rvpt_amd.build / __graft_entry__.build())."""
    global _LIB
    if _LIB is None:
        _LIB = _open(False)
    return _LIB


def load_lab() -> C.CDLL:
    """Load librvpt_hip_debug.so, the laboratory build (include/rvpt_hip_lab.h): the release ABI + selftests, host-side forms, opt-in walks, knobs, internal checks.
    A second library in the same process; contexts of the two never mix."""
    global _LAB
    if _LAB is None:
        _LAB = _open(True)
    return _LAB


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc: int, ctx=None, L=None) -> None:
    if rc != 0:
        msg = (L or load()).rvpt_hip_last_error(ctx)
        raise NativeError(rc, msg.decode() if msg else "")


def device_count() -> int:
    n = C.c_int(0)
    _check(load().rvpt_hip_device_count(C.byref(n)))
    return n.value


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """rvpt_hip_comm_unique_id: 128 bytes made by rank 0, to be handed to every rank's Context.comm_init."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().rvpt_hip_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


def comm_init_all(contexts) -> None:
    """rvpt_hip_comm_init_all: one process, one context per GPU, in rank order."""
    arr = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    _check(load().rvpt_hip_comm_init_all(arr, len(contexts)), contexts[0]._h)


def selftest_div(a, b, device: int = 0) -> np.ndarray:
    """rvpt_hip_selftest_div: the kernels' ray/plane quotient (div_dots) of two float32 arrays, evaluated on the GPU."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.zeros(a.shape, dtype=np.float32)
    _check(load_lab().rvpt_hip_selftest_div(device, _ptr(a), _ptr(b), _ptr(out), a.size), None, load_lab())
    return out


def selftest_pretest(a, den, closest, device: int = 0) -> np.ndarray:
    """rvpt_hip_selftest_pretest: per element, bit 0 = the division-free pre-test of a camera round lets (a, den, closest) through,
    bit 1 = the quotient t = div_dots(a, den) satisfies 0 < t < closest."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    den = np.ascontiguousarray(den, dtype=np.float32)
    closest = np.ascontiguousarray(closest, dtype=np.float32)
    assert a.shape == den.shape == closest.shape
    out = np.zeros(a.shape, dtype=np.uint8)
    _check(load_lab().rvpt_hip_selftest_pretest(device, _ptr(a), _ptr(den), _ptr(closest), _ptr(out), a.size), None, load_lab())
    return out


def selftest_rcp(device: int = 0) -> np.ndarray:
    """rvpt_hip_selftest_rcp: per exponent, how many binary32 b have a refined v_rcp_f32 != the correctly rounded 1/b."""
    out = np.zeros(256, dtype=np.uint64)
    _check(load_lab().rvpt_hip_selftest_rcp(device, _ptr(out)), None, load_lab())
    return out


def build_bvh(tris: np.ndarray):
    """rvpt_bvh_build: returns (nodes uint8[n_nodes,32] view-able as the node struct, prim_indices uint32[n])."""
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    n = tris.shape[0]
    nodes = np.zeros((max(2 * n - 1, 1), 8), dtype=np.uint32)
    idx = np.zeros(n, dtype=np.uint32)
    n_nodes = C.c_size_t(0)
    _check(load().rvpt_bvh_build(_ptr(tris), n, _ptr(nodes), C.byref(n_nodes), _ptr(idx)))
    return nodes[: n_nodes.value].copy(), idx


def wide_form(nodes: np.ndarray, head_shift: int):
    """rvpt_bvh_wide_form: the 4-wide regrouping of a binary tree (uint32[n, 8] or NODE_DTYPE records) that BVH contexts walk by default.
    Returns (wide float32[n_wide, 8, 4] — quads minx maxx miny maxy minz maxz head pad; view heads as uint32 —, stack_need)."""
    nodes = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 8)
    n = nodes.shape[0]
    out = np.zeros((max(n, 1), 8, 4), dtype=np.float32)
    n_wide, need = C.c_size_t(0), C.c_uint32(0)
    _check(load_lab().rvpt_bvh_wide_form(_ptr(nodes), n, int(head_shift), _ptr(out), out.shape[0], C.byref(n_wide), C.byref(need)), None, load_lab())
    return out[: n_wide.value].copy(), int(need.value)


def fast_div(x: np.ndarray, divisor: int) -> np.ndarray:
    """rvpt_hip_selftest_fast_div: x // divisor through the kernels' multiply-high division (no GPU needed)."""
    x = np.ascontiguousarray(x, dtype=np.uint32)
    q = np.zeros_like(x)
    _check(load_lab().rvpt_hip_selftest_fast_div(int(divisor), _ptr(x), _ptr(q), x.size), None, load_lab())
    return q


def camera_rects(prepared: np.ndarray, camera: np.ndarray, width: int, height: int) -> np.ndarray:
    """rvpt_camera_rects (no GPU needed): the screen rectangles of the packet kernel's camera rounds for prepared records float32[n, 16] and the
    80-byte camera block.  Returns int32[n, 4] = (x0, x1, y0, y1) in units of 16 pixels / 4 rows; x0 > x1 = no block."""
    prepared = np.ascontiguousarray(prepared, dtype=np.float32).reshape(-1, 16)
    camera = np.ascontiguousarray(camera, dtype=np.float32).reshape(20)
    out = np.zeros((prepared.shape[0], 2), dtype=np.uint32)
    _check(load_lab().rvpt_camera_rects(_ptr(prepared), prepared.shape[0], _ptr(camera), int(width), int(height), _ptr(out)), None, load_lab())
    return unpack_rects(out)


def bounce_rows(tris: np.ndarray, prepared: np.ndarray):
    """rvpt_bounce_rows (no GPU needed): the bounce cull's table for reference Triangle records float32[n, 16] and their prepared records float32[n, 16], as
    upload_scene builds it.  Returns (rows uint32[2 n, ceil(n / 32)], scene scale); scale 0 = no table for this scene."""
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    prepared = np.ascontiguousarray(prepared, dtype=np.float32).reshape(-1, 16)
    n = tris.shape[0]
    rows = np.zeros((2 * n, (n + 31) // 32), dtype=np.uint32)
    scale = C.c_double(0.0)
    _check(load_lab().rvpt_bounce_rows(_ptr(tris), _ptr(prepared), n, _ptr(rows), C.byref(scale)), None, load_lab())
    return rows, float(scale.value)


def claim_order(n_work_frame: int, group_blocks: int = 1):
    """rvpt_claim_order (no GPU needed): (order uint32[n_work_frame / 64], (groups, stride, shift)) — the tile-linear block the b-th block of the packet kernel's
    claim order is, for launches of fewer than four frames; groups == 0: this size keeps the tile-linear order."""
    order = np.zeros(n_work_frame // 64, dtype=np.uint32)
    params = np.zeros(3, dtype=np.uint32)
    _check(load_lab().rvpt_claim_order(n_work_frame, group_blocks, _ptr(order), _ptr(params)), None, load_lab())
    return order, tuple(int(x) for x in params)


def bounce_leaf_boxes(tris: np.ndarray, with_triangles: bool = False):
    """rvpt_bounce_leaf_boxes (no GPU needed): (boxes float32[n_leaves, 8] = lo.xyz, hi.xyz, 0, 0; triangles per leaf) as upload_scene builds them; with_triangles:
    also every triangle's own box float32[n, 8] (the second level)."""
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
    per = C.c_uint32(0)
    boxes = np.zeros((max(1, (tris.shape[0] + 3) // 4), 8), dtype=np.float32)  # room for leaves of four
    own = np.zeros((max(1, tris.shape[0]), 8), dtype=np.float32) if with_triangles else None
    _check(load_lab().rvpt_bounce_leaf_boxes(_ptr(tris), tris.shape[0], _ptr(boxes), C.byref(per), _ptr(own)), None, load_lab())
    leaves = boxes[: (tris.shape[0] + per.value - 1) // per.value].copy()
    return (leaves, int(per.value), own[: tris.shape[0]]) if with_triangles else (leaves, int(per.value))


def build_flags(lab: bool = False) -> int:
    """rvpt_hip_build_flags of the release (or laboratory) library: BUILD_LAB | BUILD_DEBUG_CHECKS."""
    return int((load_lab() if lab else load()).rvpt_hip_build_flags())


def unpack_rects(words: np.ndarray) -> np.ndarray:
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 2)
    return np.stack([words[:, 0] & 0xFFFF, words[:, 0] >> 16, words[:, 1] & 0xFFFF, words[:, 1] >> 16], axis=1).astype(np.int32)


NODE_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("bounds", "<f4", (6,))])

# the pieces of rvpt_hip_selftest_scene_state (include/rvpt_hip_lab.h: RVPT_HIP_STATE_*) as (number, dtype, trailing shape) by the name Context.scene_state returns them under
SCENE_STATE_PIECES = {
    "nodes": (1, NODE_DTYPE, ()), "tris": (2, np.float32, (16,)), "perm": (3, np.uint32, ()), "wide": (4, np.float32, (8, 4)), "wide_map": (5, np.uint32, (4,)),
    "refit_levels": (6, np.uint32, (2,)), "sparse_parent": (7, np.uint32, ()), "sparse_leaf_of": (8, np.uint32, ()), "sparse_dirty": (9, np.uint32, ()),
    "inv_perm": (10, np.uint32, ()), "rest": (11, np.float32, (12,)), "skin": (12, VERTEX_SKIN_DTYPE, ()), "bones": (13, np.float32, (12,)),
}
BUILT_BY = (None, "lbvh", "ploc", "sah")  # rvpt_hip_scene_state_info::built_by


class Context:
    """One rvpt_hip_ctx: one GPU, one image partition."""

    def __init__(self, width: int, height: int, device: int = 0, tile_rank: int = 0, tile_world: int = 1, flags: int = 0, lab=None):
        """lab=True: a context of the laboratory build (include/rvpt_hip_lab.h: selftests, opt-in walks, knobs, internal checks).  lab=None (default): the
        release library, unless RVPT_HIP_LAB=1 is in the environment when the context is made (experiments and tests that turn the laboratory's knobs)."""
        import os
        self.lab = bool(lab) if lab is not None else os.environ.get("RVPT_HIP_LAB") == "1"
        self._L = load_lab() if self.lab else load()
        self._h = C.c_void_p(None)
        self.width, self.height = int(width), int(height)
        self.device = int(device)
        self.tile_rank, self.tile_world, self.flags = int(tile_rank), int(tile_world), int(flags)
        self._scene_tris = None  # triangles of the last successful full upload (update_triangles)
        _check(self._L.rvpt_hip_create(C.byref(self._h), device, width, height, tile_rank, tile_world, flags), None, self._L)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.rvpt_hip_destroy(self._h)
            self._h = C.c_void_p(None)

    __del__ = close

    def upload_scene(self, nodes, tris, mats) -> None:
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 16)
        mats = np.ascontiguousarray(mats, dtype=np.float32).reshape(-1, 12)
        n_nodes = 0
        if nodes is not None:
            nodes = np.ascontiguousarray(nodes)
            n_nodes = nodes.nbytes // 32
        _check(self._L.rvpt_hip_upload_scene(self._h, _ptr(nodes), n_nodes, _ptr(tris), tris.shape[0], _ptr(mats),
                                             mats.shape[0]), self._h, self._L)
        self._scene_tris = tris.shape[0]

    def _triangle_source(self, tris, what: str):
        """(pointer, count, object to keep alive) of float32[n, 16] triangles in a numpy array or a torch tensor; a tensor on this context's device is passed as
        device memory once the stream that produced it has finished (the library copies on its own stream)."""
        if not isinstance(tris, np.ndarray) and hasattr(tris, "data_ptr"):  # a torch tensor
            import torch
            if tris.dtype != torch.float32 or tris.dim() != 2 or tris.shape[1] != 16 or not tris.is_contiguous():
                raise NativeError(ERR_INVALID, f"{what}: a contiguous float32 tensor [n, 16] is needed, got {tris.dtype} {tuple(tris.shape)}")
            if tris.is_cuda:
                if tris.device.index != self.device:
                    raise NativeError(ERR_INVALID, f"{what}: the tensor lives on device {tris.device.index}, the context on {self.device}")
                torch.cuda.current_stream(tris.device).synchronize()  # the library copies on its own stream: what produced the tensor must have finished
                return C.c_void_p(tris.data_ptr()), int(tris.shape[0]), tris
            tris = tris.numpy()
        tris = np.asarray(tris)
        if tris.dtype != np.float32 or tris.ndim != 2 or tris.shape[1] != 16:
            raise NativeError(ERR_INVALID, f"{what}: float32[n, 16] is needed, got {tris.dtype} {tris.shape}")
        tris = np.ascontiguousarray(tris)
        return _ptr(tris), tris.shape[0], tris

    def build_scene(self, tris, mats, method: str = "lbvh") -> str:
        """The build form of rvpt_hip_upload_scene (include/rvpt_hip.h): a full upload without nodes — on a BVH context the library builds the tree on the
        device (scene.build_lbvh is the same tree in numpy).  tris: float32[n, 16] in ANY order, a numpy array or — BVH contexts — a contiguous torch tensor on
        this context's device, which never visits the host; update_triangles afterwards takes the same order.  Brute-force contexts: the ordinary upload.
        method: "lbvh", "ploc" for the PLOC tree (scene.build_ploc in numpy), which falls back to the LBVH tree by the rule stated there, or "sah" for the
        binned-SAH tree of rvpt_bvh_build made on the device (scene.build_sah in numpy; no fallback).  Returns the tree the scene holds, "lbvh", "ploc" or "sah"
        (for "ploc" read from rvpt_hip_last_error, where a PLOC build that fell back says so; brute-force contexts hold no tree, take "lbvh" and "ploc" as ever,
        answer "lbvh", and refuse "sah" — at the C seam they ignore all three counts alike)."""
        if method not in ("lbvh", "ploc", "sah"):
            raise NativeError(ERR_INVALID, f"build_scene: method {method!r} is neither 'lbvh' nor 'ploc' nor 'sah'")
        if method == "sah" and (self.flags & (TRAVERSAL_BVH | TRAVERSAL_BVH_ORDERED)) == 0:
            # (the C call ignores every build count on a brute-force context; this wrapper has only ever taken the two older names there, and still does)
            raise NativeError(ERR_INVALID, "build_scene: a brute-force context builds no tree, and there method 'sah' is neither 'lbvh' nor 'ploc', the names it takes and ignores")
        count = {"lbvh": NODES_BUILD, "ploc": NODES_BUILD_PLOC, "sah": NODES_BUILD_SAH}[method]
        ptr, n, keep = self._triangle_source(tris, "build_scene")
        if not isinstance(keep, np.ndarray) and (self.flags & (TRAVERSAL_BVH | TRAVERSAL_BVH_ORDERED)) == 0:
            raise NativeError(ERR_INVALID, "build_scene: a brute-force context reads the triangles on the host, pass a host array")
        mats = np.ascontiguousarray(mats, dtype=np.float32).reshape(-1, 12)
        _check(self._L.rvpt_hip_upload_scene(self._h, None, count, ptr, n, _ptr(mats), mats.shape[0]), self._h, self._L)
        self._scene_tris = n
        del keep
        if method == "ploc" and (self.flags & (TRAVERSAL_BVH | TRAVERSAL_BVH_ORDERED)) != 0 and n > 0:
            return "lbvh" if b"LBVH tree" in (self._L.rvpt_hip_last_error(self._h) or b"") else "ploc"
        return "sah" if method == "sah" else "lbvh"

    def update_triangles(self, tris, rebuild_above=None, indices=None):
        """The update form of rvpt_hip_upload_scene (include/rvpt_hip.h): the scene's triangles have moved — same count, same tree topology as the last full
        upload, in the order that upload took them: the leaf order after upload_scene, the caller's own order after build_scene.
        Only vert0..vert2 are taken; material rows, materials and the tree's structure stay, every box of the tree is refitted on the
        device (scene.refit_bvh is the same on the host).  Frames in flight finish on the old geometry; restarting the accumulation is the caller's business.
        tris: float32[n, 16], a numpy array or — BVH contexts — a contiguous torch tensor on this context's device, which never visits the host.

        rebuild_above: None is the plain form and returns None.  A number is the GUARDED form (RVPT_HIP_NODES_UPDATE_GUARDED): after the refit the library
        computes the tree's SAH cost on the device (scene.tree_cost is the same in numpy) and, when it exceeds rebuild_above x the cost of the tree as it was built,
        rebuilds with the method of the build_scene that made it.  A float >= 1 is rounded to thousandths (at most 65.535); math.inf only reports.  Returns an
        UpdateReport (cost, base_cost, ratio, rebuilt, tree); on a brute-force context, which holds no tree, the plain update happens and None is returned.

        indices: None, or the SPARSE form (RVPT_HIP_NODES_UPDATE_SPARSE): tris[j] replaces the vertices of stored triangle indices[j] (the same order rule), and on a
        BVH context only the boxes on the paths from the touched leaves to the root are recomputed (scene.refit_bvh(..., touched=) is the same on the host); every
        other box stays as it is.  A numpy integer array of k entries beside a host `tris` of k rows, or a contiguous 1-D torch.int32 tensor on this context's device
        beside a device `tris`.  No index twice, none outside the scene.  Not together with rebuild_above.  An empty list changes nothing.  Returns None."""
        if indices is not None:
            return self._update_sparse(tris, rebuild_above, indices)
        ptr, n, keep = self._triangle_source(tris, "update_triangles")
        count = 0
        if rebuild_above is not None:
            count = nodes_update_guarded(_guard_permille(rebuild_above, "update_triangles"))
        if n == 0:  # (in the C form a call without triangles is a full upload of the empty scene)
            if self._scene_tris != 0:
                raise NativeError(ERR_INVALID, "update_triangles: no triangles given" + (" before any upload_scene" if self._scene_tris is None else f", the uploaded scene has {self._scene_tris}"))
            return None
        _check(self._L.rvpt_hip_upload_scene(self._h, None, count, ptr, n, None, 0), self._h, self._L)
        del keep
        if count == 0 or (self.flags & (TRAVERSAL_BVH | TRAVERSAL_BVH_ORDERED)) == 0:
            return None
        return parse_update_report((self._L.rvpt_hip_last_error(self._h) or b"").decode())

    def _update_sparse(self, tris, rebuild_above, indices) -> None:
        if rebuild_above is not None:
            raise NativeError(ERR_INVALID, "update_triangles: indices (the sparse form) and rebuild_above (the guarded form) do not combine")
        ptr, n, keep = self._triangle_source(tris, "update_triangles")
        if not isinstance(indices, np.ndarray) and hasattr(indices, "data_ptr"):  # a torch tensor
            import torch
            if indices.dtype != torch.int32 or indices.dim() != 1 or not indices.is_contiguous():
                raise NativeError(ERR_INVALID, f"update_triangles: indices as a tensor are contiguous 1-D torch.int32, got {indices.dtype} {tuple(indices.shape)}")
            if indices.is_cuda != (not isinstance(keep, np.ndarray)):
                raise NativeError(ERR_INVALID, "update_triangles: indices and triangles are both host arrays or both tensors on the context's device, got a mixed pair")
            if indices.is_cuda:
                if indices.device.index != self.device:
                    raise NativeError(ERR_INVALID, f"update_triangles: the index tensor lives on device {indices.device.index}, the context on {self.device}")
                torch.cuda.current_stream(indices.device).synchronize()
                iptr, k, ikeep = C.c_void_p(indices.data_ptr()), int(indices.shape[0]), indices
            else:
                indices = indices.numpy()
        if isinstance(indices, np.ndarray) or not hasattr(indices, "data_ptr"):
            idx = np.asarray(indices)
            if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
                raise NativeError(ERR_INVALID, f"update_triangles: indices are a 1-D integer array, got {idx.dtype} {idx.shape}")
            if not isinstance(keep, np.ndarray):
                raise NativeError(ERR_INVALID, "update_triangles: indices and triangles are both host arrays or both tensors on the context's device, got a mixed pair")
            if idx.size and (int(idx.min()) < 0 or int(idx.max()) > 0xFFFFFFFF):
                bad = int(np.flatnonzero((idx < 0) | (idx > 0xFFFFFFFF))[0])
                raise NativeError(ERR_INVALID, f"update_triangles: indices[{bad}] = {int(idx[bad])} is not a triangle index")
            ikeep = np.ascontiguousarray(idx, dtype=np.uint32)
            iptr, k = _ptr(ikeep), int(ikeep.shape[0])
        if k == 0:
            return None
        if k != n:
            raise NativeError(ERR_INVALID, f"update_triangles: {k} indices for {n} triangles")
        _check(self._L.rvpt_hip_upload_scene(self._h, iptr, NODES_UPDATE_SPARSE, ptr, n, None, 0), self._h, self._L)
        del keep, ikeep
        return None

    def pose_parts(self, moves, rebuild_above=None):
        """The POSE UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): every move names a range of triangles [first, first + count) — in the order
        update_triangles takes: the leaf order after upload_scene, the caller's own order after build_scene — and a 3x4 matrix; the device poses those triangles
        from the REST POSE it keeps (the vertices as the last call of any other form left them; two poses of one part do not compose) and recomputes only the boxes
        above them.  scene.pose_parts is the same on the host, bit for bit.  moves: a structured array of PART_MOVE_DTYPE, or a sequence of
        (first, count, matrix) with a 3x4 matrix or a 4x4 matrix whose last row is 0 0 0 1.  A malformed matrix or a negative `first` is refused here; ranges that
        overlap or leave the scene are left to the library, which names them.  An empty list changes nothing.

        rebuild_above: None is the plain form and returns None.  A number is the GUARDED form (RVPT_HIP_NODES_UPDATE_POSE_GUARDED): behind the pose the library
        computes the tree's SAH cost on the device and, when it exceeds rebuild_above x the cost of the tree as it was built, rebuilds with the method of the
        build_scene that made it; the rest pose follows the triangles through the rebuild, so later poses start from the same rest pose.  A float >= 1 is rounded
        to thousandths (at most 65.535); math.inf only reports.  Returns an UpdateReport, whose `tree` names the tree the scene holds after a rebuild; on a
        brute-force context, which holds no tree, the plain pose happens and None is returned."""
        from . import scene
        count = NODES_UPDATE_POSE if rebuild_above is None else nodes_update_pose_guarded(_guard_permille(rebuild_above, "pose_parts"))
        try:
            rec = scene.part_moves(moves)
        except (ValueError, TypeError) as e:
            raise NativeError(ERR_INVALID, f"pose_parts: {e}") from None
        if rec.shape[0] == 0:
            return None
        _check(self._L.rvpt_hip_upload_scene(self._h, _ptr(rec), count, None, rec.shape[0], None, 0), self._h, self._L)
        if rebuild_above is None or (self.flags & (TRAVERSAL_BVH | TRAVERSAL_BVH_ORDERED)) == 0:
            return None
        return parse_update_report((self._L.rvpt_hip_last_error(self._h) or b"").decode())

    def _device_tensor(self, t, what: str, words: int):
        """(pointer, rows) of a contiguous float32 / int32 / uint8 torch tensor on this context's device whose rows are `words` 4-byte words: device memory passed
        as it is once the stream that wrote it has finished.  None for a tensor on the host (the caller then takes its numpy view)."""
        import torch
        if not t.is_cuda:
            return None
        if t.device.index != self.device:
            raise NativeError(ERR_INVALID, f"{what}: the tensor lives on device {t.device.index}, the context on {self.device}")
        nbytes = t.numel() * t.element_size()
        if not t.is_contiguous() or t.element_size() not in (1, 4) or nbytes % (4 * words):
            raise NativeError(ERR_INVALID, f"{what}: a contiguous tensor of {4 * words}-byte records is needed, got {t.dtype} {tuple(t.shape)}")
        torch.cuda.current_stream(t.device).synchronize()  # the library works on its own stream: what wrote the tensor must have finished
        return C.c_void_p(t.data_ptr()), nbytes // (4 * words)

    def bind_skin(self, skin, weights=None) -> None:
        """The BIND of rvpt_hip_upload_scene (include/rvpt_hip.h): four bone indices and four weights per vertex, three records per triangle in the order
        update_triangles takes, kept by the library for skin().  skin: what scene.vertex_skins takes — a VERTEX_SKIN_DTYPE array, or indices[n, 3, 4] beside
        weights[n, 3, 4] — or, on a BVH context, a contiguous torch tensor on this context's device holding the 32-byte records (int32 / float32 [3 n, 8], or
        uint8 [3 n, 32]), which never visits the host.  Moves nothing; a second bind replaces the first; an upload_scene or build_scene drops the binding."""
        from . import scene
        if weights is None and not isinstance(skin, (np.ndarray, tuple, list)) and hasattr(skin, "data_ptr"):
            dev = self._device_tensor(skin, "bind_skin", 8)
            if dev is not None:
                ptr, records = dev
                if records % 3:
                    raise NativeError(ERR_INVALID, f"bind_skin: {records} records are not three per triangle")
                _check(self._L.rvpt_hip_upload_scene(self._h, ptr, NODES_BIND_SKIN, None, records // 3, None, 0), self._h, self._L)
                return None
            skin = skin.numpy().view(np.uint8).reshape(-1).view(VERTEX_SKIN_DTYPE)
        try:
            rec = scene.vertex_skins(skin, weights)
        except (ValueError, TypeError) as e:
            raise NativeError(ERR_INVALID, f"bind_skin: {e}") from None
        _check(self._L.rvpt_hip_upload_scene(self._h, _ptr(rec), NODES_BIND_SKIN, None, rec.shape[0] // 3, None, 0), self._h, self._L)
        return None

    def skin(self, bones, rebuild_above=None):
        """The SKIN UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): linear blend skinning — every vertex is posed FROM THE REST POSE (the pose update's) by
        the four weighted matrices its bound record names, and every box of the tree is refitted as after update_triangles.  scene.skin_triangles is the same
        on the host, bit for bit.  bones: float32[k, 3, 4] or [k, 12], [k, 4, 4] with last rows 0 0 0 1, or — BVH contexts — a contiguous float32 torch tensor
        [k, 3, 4] / [k, 12] on this context's device, which never visits the host.  Needs a bind_skin first and more bones than its largest index.

        rebuild_above: None is the plain form and returns None.  A number is the GUARDED form (RVPT_HIP_NODES_UPDATE_SKIN_GUARDED): behind the skin the library
        computes the tree's SAH cost on the device and, when it exceeds rebuild_above x the cost of the tree as it was built, rebuilds with the method of the
        build_scene that made it; the rest pose follows the triangles through the rebuild and the binding stays, so later skins pose from the same rest pose
        through the same weights.  A float >= 1 is rounded to thousandths (at most 65.535); math.inf only reports.  Returns an UpdateReport, whose `tree` names
        the tree the scene holds after a rebuild; on a brute-force context, which holds no tree, the plain skin happens and None is returned."""
        from . import scene
        count = NODES_UPDATE_SKIN if rebuild_above is None else nodes_update_skin_guarded(_guard_permille(rebuild_above, "skin"))
        if not isinstance(bones, np.ndarray) and hasattr(bones, "data_ptr"):
            import torch
            if bones.dtype != torch.float32 or tuple(bones.shape[1:]) not in ((3, 4), (12,)):
                raise NativeError(ERR_INVALID, f"skin: a float32 tensor [k, 3, 4] or [k, 12] is needed, got {bones.dtype} {tuple(bones.shape)}")
            dev = self._device_tensor(bones, "skin", 12)
            if dev is not None:
                _check(self._L.rvpt_hip_upload_scene(self._h, dev[0], count, None, dev[1], None, 0), self._h, self._L)
                return _report_of(self, rebuild_above)
            bones = bones.numpy()
        try:
            m = scene.bone_matrices(bones)
        except (ValueError, TypeError) as e:
            raise NativeError(ERR_INVALID, f"skin: {e}") from None
        _check(self._L.rvpt_hip_upload_scene(self._h, _ptr(m), count, None, m.shape[0], None, 0), self._h, self._L)
        return _report_of(self, rebuild_above)

    def set_frame(self, settings: np.ndarray, camera: np.ndarray) -> None:
        settings = np.ascontiguousarray(settings)
        camera = np.ascontiguousarray(camera, dtype=np.float32).reshape(20)
        if settings.nbytes != 40:
            raise NativeError(ERR_INVALID, "settings block must be 40 bytes")
        _check(self._L.rvpt_hip_set_frame(self._h, _ptr(settings), _ptr(camera)), self._h, self._L)

    def set_frame_fast(self, rs, camera: np.ndarray) -> None:
        """set_frame from a RenderSettings object without per-call allocations (the per-frame host loop)."""
        buf = getattr(self, "_rs_buf", None)
        if buf is None:
            buf = self._rs_buf = np.zeros(10, dtype=np.int32)
            self._rs_u32, self._rs_f32 = buf.view(np.uint32), buf.view(np.float32)
            self._rs_ptr = buf.ctypes.data_as(C.c_void_p)
        buf[0], buf[1] = rs.max_bounces, rs.aa
        self._rs_u32[2] = rs.current_frame & 0xFFFFFFFF
        buf[3], buf[4], buf[5], buf[6], buf[7] = (rs.camera_mode, rs.top_left_render_mode, rs.top_right_render_mode,
                                                  rs.bottom_left_render_mode, rs.bottom_right_render_mode)
        self._rs_f32[8], self._rs_f32[9] = rs.split_ratio
        cam = getattr(self, "_cam_last", None)
        if cam is None or cam[0] is not camera:
            c = np.ascontiguousarray(camera, dtype=np.float32).reshape(20)
            cam = self._cam_last = (camera, c, c.ctypes.data_as(C.c_void_p))
        rc = self._L.rvpt_hip_set_frame(self._h, self._rs_ptr, cam[2])
        if rc:
            _check(rc, self._h, self._L)

    def dispatch(self) -> None:
        rc = self._L.rvpt_hip_dispatch(self._h)
        if rc:
            _check(rc, self._h, self._L)

    def dispatch_frames(self, n_frames: int) -> None:
        """n consecutive frames starting at the last set_frame()'s current_frame, as one launch."""
        rc = self._L.rvpt_hip_dispatch_frames(self._h, n_frames)
        if rc:
            _check(rc, self._h, self._L)

    def wait(self) -> None:
        _check(self._L.rvpt_hip_wait(self._h), self._h, self._L)

    def wait_for(self, timeout_s: float) -> bool:
        """True when everything dispatched so far has finished within timeout_s, False if still pending."""
        rc = self._L.rvpt_hip_wait_for(self._h, int(timeout_s * 1e9))
        if rc < 0:
            _check(rc, self._h, self._L)
        return rc == 0

    def query(self) -> bool:
        """True while work is pending."""
        rc = self._L.rvpt_hip_query(self._h)
        if rc < 0:
            _check(rc, self._h, self._L)
        return rc == 1

    def read(self, fmt: int = FORMAT_RGBA32F) -> np.ndarray:
        dt = np.float32 if fmt == FORMAT_RGBA32F else np.uint8
        out = np.empty((self.height, self.width, 4), dtype=dt)
        _check(self._L.rvpt_hip_read(self._h, fmt, _ptr(out), out.nbytes), self._h, self._L)
        return out

    def _frame_buffer(self, buf, fmt: int, what: str):
        """(pointer, bytes, object to keep alive) of a whole frame in a numpy array or a torch tensor — contiguous float32[h, w, 4] (FORMAT_RGBA32F) or
        uint8[h, w, 4] (FORMAT_RGBA8_UNORM); resolved the way _triangle_source resolves triangles: a tensor on this context's device is passed as device memory
        once the stream that last touched it has finished, and torch is imported only when a tensor is given.  Checked here, before the call."""
        if fmt in (FORMAT_RAY_HITS, FORMAT_RAY_PATHS) or (isinstance(fmt, int) and (16 <= fmt <= 16 + PATH_MODE_KAJIYA or 33 <= fmt <= 32 + RAY_MAX_HITS)):  # known formats, but of records and not of a frame
            raise NativeError(ERR_INVALID, f"{what}: format {fmt} holds query records, not a frame: use trace_rays_into / trace_paths_into")
        if fmt == FORMAT_RAY_CROSSINGS:
            raise NativeError(ERR_INVALID, f"{what}: format {fmt} holds query records, not a frame: use count_crossings_into")
        if fmt == FORMAT_BOX_OVERLAPS or (isinstance(fmt, int) and 65 <= fmt <= 64 + BOX_MAX_GROUP):
            raise NativeError(ERR_INVALID, f"{what}: format {fmt} holds query records, not a frame: use box_overlaps_into")
        if fmt == FORMAT_SPHERE_SWEEPS:
            raise NativeError(ERR_INVALID, f"{what}: format {fmt} holds query records, not a frame: use sweep_spheres_into")
        if fmt == FORMAT_TRIANGLES:
            raise NativeError(ERR_INVALID, f"{what}: format {fmt} holds the stored triangle rows, not a frame: use read_triangles / read_triangles_into")
        if fmt == FORMAT_SURFACE_POINTS:
            raise NativeError(ERR_INVALID, f"{what}: format {fmt} holds surface records, not a frame: use surface_points / surface_points_into")
        if fmt not in (FORMAT_RGBA32F, FORMAT_RGBA8_UNORM):
            raise NativeError(ERR_INVALID, f"{what}: unknown format {fmt}")
        name, size = ("float32", 4) if fmt == FORMAT_RGBA32F else ("uint8", 1)
        shape, need = (self.height, self.width, 4), self.height * self.width * 4 * size
        is_tensor = not isinstance(buf, np.ndarray) and hasattr(buf, "data_ptr")
        if not is_tensor and not isinstance(buf, np.ndarray):
            raise NativeError(ERR_INVALID, f"{what}: a numpy array or a torch tensor is needed, got {type(buf).__name__}")
        if is_tensor:
            import torch
            dtype_ok, nbytes, contiguous = buf.dtype == getattr(torch, name), buf.numel() * buf.element_size(), buf.is_contiguous()
        else:
            dtype_ok, nbytes, contiguous = buf.dtype == np.dtype(name), buf.nbytes, buf.flags.c_contiguous
        if not dtype_ok:
            raise NativeError(ERR_INVALID, f"{what}: {name}[{self.height}, {self.width}, 4] is needed for format {fmt}, got {buf.dtype}")
        if nbytes < need:
            raise NativeError(ERR_SIZE, f"{what}: holds {nbytes} bytes, frame needs {need}")
        if tuple(buf.shape) != shape or not contiguous:
            raise NativeError(ERR_INVALID, f"{what}: a contiguous {name}{list(shape)} is needed, got {tuple(buf.shape)}{'' if contiguous else ', not contiguous'}")
        if is_tensor:
            if buf.is_cuda:
                if buf.device.index != self.device:
                    raise NativeError(ERR_INVALID, f"{what}: the tensor lives on device {buf.device.index}, the context on {self.device}")
                torch.cuda.current_stream(buf.device).synchronize()  # the library works on its own stream: what touched the tensor last must have finished
                return C.c_void_p(buf.data_ptr()), need, buf
            buf = buf.numpy()  # (shares the tensor's memory)
        return _ptr(buf), need, buf

    def read_into(self, dst, fmt: int = FORMAT_RGBA32F):
        """rvpt_hip_read into the caller's memory: `dst` is a contiguous torch tensor on this context's device — the frame then never visits the host: the
        un-tiling kernel writes it in place, a view that is only 4-byte aligned included — or a numpy array (the host read); float32[h, w, 4] for
        FORMAT_RGBA32F, uint8[h, w, 4] for FORMAT_RGBA8_UNORM.  The bytes are those read() returns.  On return the library's stream has finished writing: the
        tensor may be used on any stream.  Returns dst."""
        ptr, nbytes, keep = self._frame_buffer(dst, fmt, "read_into")
        _check(self._L.rvpt_hip_read(self._h, fmt, ptr, nbytes), self._h, self._L)
        del keep
        return dst

    def trace_rays(self, org, dir, tmax=math.inf, any_hit=False, hits=None) -> np.ndarray:
        """Closest (any_hit: first accepted) hit of the rays org[n, 3] + t dir[n, 3], 0 < t < tmax, against the uploaded scene — include/rvpt_hip.h: RAY QUERIES
        has the order a query walks and the numbering of prim.  tmax and any_hit are scalars or one value per ray.  Returns RAY_HIT_DTYPE[n]: t, prim, u, v of
        the hit, prim == NO_PRIM where there is none.  hits=k (1 .. RAY_MAX_HITS) asks for the k nearest hits of every ray (K-NEAREST RAY QUERIES; any_hit:
        the first k accepted) and returns RAY_HIT_DTYPE[n, k], record j of a row the j-th hit, prim == NO_PRIM from the first slot no hit fills; the ray is
        repeated in every record's in fields."""
        if hits is not None:
            FORMAT_RAY_HITS_NEAREST(hits)  # (before anything else: a refusal needs no arrays)
        org = np.asarray(org, dtype=np.float32).reshape(-1, 3)
        dirv = np.asarray(dir, dtype=np.float32).reshape(-1, 3)
        if org.shape != dirv.shape:
            raise NativeError(ERR_INVALID, f"trace_rays: {org.shape[0]} origins, {dirv.shape[0]} directions")
        rec = np.zeros(org.shape[0], dtype=RAY_HIT_DTYPE)
        rec["org"], rec["dir"] = org, dirv
        rec["tmax"] = np.asarray(tmax, dtype=np.float32)
        rec["flags"] = np.where(np.asarray(any_hit, dtype=bool), RAY_ANY_HIT, 0).astype(np.uint32)
        if hits is not None:
            return self.trace_rays_into(np.ascontiguousarray(np.repeat(rec[:, None], int(hits), axis=1)), hits=hits)
        return self.trace_rays_into(rec)

    def trace_rays_into(self, records, hits=None):
        """rvpt_hip_read with FORMAT_RAY_HITS in the caller's memory: `records` is a contiguous RAY_HIT_DTYPE array, or a contiguous float32 torch tensor [n, 12]
        (48-byte records) on the host or on this context's device — resolved the way _frame_buffer resolves frames; device records never visit the host.  The
        in fields stay as they are, the out fields are written.  Returns records.  hits=k (1 .. RAY_MAX_HITS): the call goes out with
        FORMAT_RAY_HITS_NEAREST(k) and `records` holds n groups of k records — a RAY_HIT_DTYPE array shaped (n * k,) or (n, k), or a tensor [n * k, 12]; record
        0 of a group carries the ray, the out quad of record j receives the j-th hit.  A record count that is no multiple of k raises before any call."""
        if hits is None:
            return self._query_into(records, FORMAT_RAY_HITS, RAY_HIT_DTYPE, "trace_rays_into", "RAY_HIT_DTYPE")
        fmt = FORMAT_RAY_HITS_NEAREST(hits)
        k = int(hits)
        if isinstance(records, np.ndarray):
            if records.ndim == 2 and records.shape[1] != k:
                raise NativeError(ERR_INVALID, f"trace_rays_into: hits={k} needs RAY_HIT_DTYPE[n, {k}] or [n * {k}], got shape {tuple(records.shape)}")
            count = records.size
        else:
            count = int(records.shape[0]) if hasattr(records, "data_ptr") and records.dim() == 2 else 0  # (_query_into refuses what is no tensor [n, 12])
        if count % k:
            raise NativeError(ERR_INVALID, f"trace_rays_into: {count} records are not a multiple of hits={k}: a ray takes a group of {k} records")
        return self._query_into(records, fmt, RAY_HIT_DTYPE, "trace_rays_into", "RAY_HIT_DTYPE")

    def count_crossings(self, org, dir, tmax=math.inf) -> np.ndarray:
        """Front and back hit counts of the rays org[n, 3] + t dir[n, 3], 0 < t < tmax, against the uploaded scene — include/rvpt_hip.h: RAY CROSSINGS has the
        set that is counted and the facing rule.  tmax is a scalar or one value per ray.  Returns RAY_CROSSINGS_DTYPE[n]: front, back, and the smallest and
        largest accepted t; with no crossing front = back = 0, t_near = tmax and t_far = 0."""
        org = np.asarray(org, dtype=np.float32).reshape(-1, 3)
        dirv = np.asarray(dir, dtype=np.float32).reshape(-1, 3)
        if org.shape != dirv.shape:
            raise NativeError(ERR_INVALID, f"count_crossings: {org.shape[0]} origins, {dirv.shape[0]} directions")
        tmax = np.asarray(tmax, dtype=np.float32)
        if tmax.ndim > 1 or (tmax.ndim == 1 and tmax.shape[0] != org.shape[0]):
            raise NativeError(ERR_INVALID, f"count_crossings: {org.shape[0]} rays, tmax of shape {tuple(tmax.shape)}")
        rec = np.zeros(org.shape[0], dtype=RAY_CROSSINGS_DTYPE)
        rec["org"], rec["dir"], rec["tmax"] = org, dirv, tmax
        return self.count_crossings_into(rec)

    def count_crossings_into(self, records):
        """rvpt_hip_read with FORMAT_RAY_CROSSINGS in the caller's memory: `records` is a contiguous RAY_CROSSINGS_DTYPE array, or a contiguous float32 torch
        tensor [n, 12] (48-byte records; front and back are the bits of their floats) on the host or on this context's device, as for trace_rays_into.  The in
        fields stay as they are, the out fields are written.  Returns records."""
        return self._query_into(records, FORMAT_RAY_CROSSINGS, RAY_CROSSINGS_DTYPE, "count_crossings_into", "RAY_CROSSINGS_DTYPE")

    def _query_into(self, records, fmt: int, dtype, what: str, dtype_name: str):
        is_tensor = not isinstance(records, np.ndarray) and hasattr(records, "data_ptr")
        if is_tensor:
            import torch
            if records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != 12 or not records.is_contiguous():
                raise NativeError(ERR_INVALID, f"{what}: a contiguous float32 tensor [n, 12] is needed, got {records.dtype} {tuple(records.shape)}")
            nbytes = int(records.shape[0]) * 48
            if records.is_cuda:
                if records.device.index != self.device:
                    raise NativeError(ERR_INVALID, f"{what}: the tensor lives on device {records.device.index}, the context on {self.device}")
                torch.cuda.current_stream(records.device).synchronize()  # the library works on its own stream: what wrote the rays must have finished
                ptr = C.c_void_p(records.data_ptr())
            else:
                ptr = _ptr(records.numpy())  # (shares the tensor's memory)
        elif isinstance(records, np.ndarray):
            if records.dtype != dtype or not records.flags.c_contiguous or not records.flags.writeable:
                raise NativeError(ERR_INVALID, f"{what}: a contiguous writeable {dtype_name} array is needed, got {records.dtype}")
            ptr, nbytes = _ptr(records), records.nbytes
        else:
            raise NativeError(ERR_INVALID, f"{what}: a numpy array or a torch tensor is needed, got {type(records).__name__}")
        _check(self._L.rvpt_hip_read(self._h, fmt, ptr, nbytes), self._h, self._L)
        return records

    def trace_paths(self, org, dir, seed, max_bounces, mode=PATH_MODE_KAJIYA) -> np.ndarray:
        """integrator_Kajiya's radiance along the rays org[n, 3] + t dir[n, 3] against the uploaded scene — include/rvpt_hip.h: PATH QUERIES.  seed (the RNG state
        a path starts from) and max_bounces (1 .. PATH_MAX_BOUNCES) are scalars or one value per ray.  Returns RAY_PATH_DTYPE[n]: radiance, and the segments the
        path traced; both 0 for an invalid record.  mode (0 .. 9, one for the whole call) names another integrator of compute_pass.comp for every record:
        max_bounces is then what that integrator reads as render_settings.max_bounces (the occlusion samples of mode 5; modes 0-4 and 6 ignore it, but the
        validity rule does not), and the segments count shadow and occlusion queries too.  A mode outside 0 .. 9 raises before any call."""
        fmt = format_ray_paths_mode(mode)  # (before anything else: a refusal needs no arrays)
        org = np.asarray(org, dtype=np.float32).reshape(-1, 3)
        dirv = np.asarray(dir, dtype=np.float32).reshape(-1, 3)
        if org.shape != dirv.shape:
            raise NativeError(ERR_INVALID, f"trace_paths: {org.shape[0]} origins, {dirv.shape[0]} directions")
        n = org.shape[0]
        per_ray = {}
        for name, value in (("seed", seed), ("max_bounces", max_bounces)):
            value = np.asarray(value)
            if value.ndim > 1 or (value.ndim == 1 and value.shape[0] != n):
                raise NativeError(ERR_INVALID, f"trace_paths: {n} rays, {name} of shape {tuple(value.shape)}")
            if value.dtype.kind not in "iu" or (value.size and (value.min() < 0 or value.max() > 0xFFFFFFFF)):
                raise NativeError(ERR_INVALID, f"trace_paths: {name} must be integers in [0, 2^32), got {value.dtype}")
            per_ray[name] = value.astype(np.uint32)
        rec = np.zeros(n, dtype=RAY_PATH_DTYPE)
        rec["org"], rec["dir"] = org, dirv
        rec["seed"], rec["max_bounces"] = per_ray["seed"], per_ray["max_bounces"]
        return self.trace_paths_into(rec, mode=fmt - 16)

    def trace_paths_into(self, records, mode=PATH_MODE_KAJIYA):
        """rvpt_hip_read with FORMAT_RAY_PATHS in the caller's memory: `records` is a contiguous RAY_PATH_DTYPE array, or a contiguous float32 torch tensor
        [n, 12] (48-byte records; seed, max_bounces and segments are the bits of their floats) on the host or on this context's device, as for trace_rays_into.
        The in fields stay as they are, the out fields are written.  Returns records.  mode (0 .. 9) as for trace_paths: the call then goes out with
        format_ray_paths_mode(mode); the default, 9, is FORMAT_RAY_PATHS itself."""
        fmt = format_ray_paths_mode(mode)
        if fmt == 16 + PATH_MODE_KAJIYA:
            fmt = FORMAT_RAY_PATHS  # (the same kernels and bytes under either value: the form's first name is kept on the wire)
        return self._query_into(records, fmt, RAY_PATH_DTYPE, "trace_paths_into", "RAY_PATH_DTYPE")

    def closest_points(self, points, max_dist=math.inf, k=None) -> np.ndarray:
        """The nearest point of the uploaded mesh to every point of points[n, 3] — include/rvpt_hip.h: NEAREST POINTS has the definition, the arithmetic and the
        numbering of prim.  max_dist, a scalar or one value per point, is a DISTANCE: it is squared here in float32 (max_dist * max_dist, one rounding) into the
        record's max_d2, the bound the library compares squared distances against; +inf searches without a bound, a negative or NaN max_dist makes the record
        invalid.  Returns POINT_HIT_DTYPE[n]: closest, d2 (squared: np.sqrt(rec["d2"]) is the distance), prim, u, v, region; prim == NO_PRIM where no triangle is
        within the bound.  k (1 .. POINT_MAX_NEAREST) asks for the k nearest triangles of every point (K-NEAREST POINTS: the first k candidates by (d2, prim))
        and returns POINT_HIT_DTYPE[n, k], record j of a row the j-th entry, prim == NO_PRIM from the first slot no triangle fills; the point and the bound are
        repeated in every record's in fields."""
        if k is not None:
            FORMAT_NEAREST_POINTS_K(k)  # (before anything else: a refusal needs no arrays)
        pts = np.asarray(points, dtype=np.float32)
        if pts.ndim == 0 or pts.size % 3 or (pts.ndim > 1 and pts.shape[-1] != 3):
            raise NativeError(ERR_INVALID, f"closest_points: points[n, 3] are needed, got shape {tuple(pts.shape)}")
        pts = pts.reshape(-1, 3)
        dist = np.asarray(max_dist, dtype=np.float32)
        if dist.ndim > 1 or (dist.ndim == 1 and dist.shape[0] != pts.shape[0]):
            raise NativeError(ERR_INVALID, f"closest_points: {pts.shape[0]} points, max_dist of shape {tuple(dist.shape)}")
        rec = np.zeros(pts.shape[0], dtype=POINT_HIT_DTYPE)
        rec["point"] = pts
        with np.errstate(all="ignore"):
            rec["max_d2"] = np.where(dist < 0, np.float32(-1), dist * dist)  # (a negative distance must not square into a valid bound)
        if k is not None:
            return self.closest_points_into(np.ascontiguousarray(np.repeat(rec[:, None], int(k), axis=1)), k=k)
        return self.closest_points_into(rec)

    def closest_points_into(self, records, k=None):
        """rvpt_hip_read with FORMAT_NEAREST_POINTS in the caller's memory: `records` is a contiguous POINT_HIT_DTYPE array, or a contiguous float32 torch tensor
        [n, 12] (48-byte records; prim and region are the bits of their floats) on the host or on this context's device, as for trace_rays_into.  The in fields
        (point, max_d2 — a SQUARED distance) stay as they are, the out fields are written.  Returns records.  k (1 .. POINT_MAX_NEAREST): the call goes out with
        FORMAT_NEAREST_POINTS_K(k) and `records` holds n groups of k records — a POINT_HIT_DTYPE array shaped (n * k,) or (n, k), or a tensor [n * k, 12];
        record 0 of a group carries the point and the bound, the out fields of record j receive the j-th entry.  A record count that is no multiple of k raises
        before any call."""
        if k is None:
            return self._query_into(records, FORMAT_NEAREST_POINTS, POINT_HIT_DTYPE, "closest_points_into", "POINT_HIT_DTYPE")
        fmt = FORMAT_NEAREST_POINTS_K(k)
        k = int(k)
        if isinstance(records, np.ndarray):
            if records.ndim > 2 or (records.ndim == 2 and records.shape[1] != k):
                raise NativeError(ERR_INVALID, f"closest_points_into: k={k} needs POINT_HIT_DTYPE[n, {k}] or [n * {k}], got shape {tuple(records.shape)}")
            count = records.size
        else:
            count = int(records.shape[0]) if hasattr(records, "data_ptr") and records.dim() == 2 else 0  # (_query_into refuses what is no tensor [n, 12])
        if count % k:
            raise NativeError(ERR_INVALID, f"closest_points_into: {count} records are not a multiple of k={k}: a point takes a group of {k} records")
        return self._query_into(records, fmt, POINT_HIT_DTYPE, "closest_points_into", "POINT_HIT_DTYPE")

    def box_overlaps(self, lo, hi, prim_from=0, k=1) -> np.ndarray:
        """How many triangles of the uploaded mesh meet each of the closed boxes [lo[n, 3], hi[n, 3]], and which — include/rvpt_hip.h: BOX OVERLAPS has the
        set, the test and the numbering of prim.  prim_from, a scalar or one value per box, leaves out every triangle whose number is below it (paging: ask
        again with the last listed number + 1).  Returns BOX_OVERLAP_DTYPE[n, k]: rec["count"][:, 0] is the count; the 4k - 1 smallest numbers, ascending and
        NO_PRIM past the last, are rec["prim"][:, 0] followed by the out quads of records 1 .. k - 1 (box_overlap_lists puts them side by side)."""
        FORMAT_BOX_OVERLAPS_K(k)  # (before anything else: a refusal needs no arrays)
        lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
        if lo.ndim == 0 or lo.size % 3 or lo.shape != hi.shape or (lo.ndim > 1 and lo.shape[-1] != 3):
            raise NativeError(ERR_INVALID, f"box_overlaps: lo[n, 3] and hi[n, 3] are needed, got shapes {tuple(lo.shape)} and {tuple(hi.shape)}")
        lo, hi = lo.reshape(-1, 3), hi.reshape(-1, 3)
        first = np.asarray(prim_from, dtype=np.uint32)
        if first.ndim > 1 or (first.ndim == 1 and first.shape[0] != lo.shape[0]):
            raise NativeError(ERR_INVALID, f"box_overlaps: {lo.shape[0]} boxes, prim_from of shape {tuple(first.shape)}")
        rec = np.zeros((lo.shape[0], int(k)), dtype=BOX_OVERLAP_DTYPE)
        rec["lo"][:, 0], rec["hi"][:, 0], rec["prim_from"][:, 0] = lo, hi, first
        return self.box_overlaps_into(rec, k=k)

    def box_overlaps_into(self, records, k=1):
        """rvpt_hip_read with FORMAT_BOX_OVERLAPS (k = 1) or FORMAT_BOX_OVERLAPS_K(k) in the caller's memory: `records` holds n groups of k records — a contiguous
        BOX_OVERLAP_DTYPE array shaped (n * k,) or (n, k), or a contiguous float32 torch tensor [n * k, 12] (48-byte records; prim_from, count and the numbers are
        the bits of their floats) on the host or on this context's device, as for trace_rays_into.  Record 0 of a group carries the box; every in quad stays as it
        is, the out quads are written.  Returns records.  A record count that is no multiple of k raises before any call."""
        fmt = FORMAT_BOX_OVERLAPS_K(k)
        k = int(k)
        if k == 1:
            fmt = FORMAT_BOX_OVERLAPS  # (the same kernels and bytes under either value: the form's first name is kept on the wire)
        if isinstance(records, np.ndarray):
            if records.ndim > 2 or (records.ndim == 2 and records.shape[1] != k):
                raise NativeError(ERR_INVALID, f"box_overlaps_into: k={k} needs BOX_OVERLAP_DTYPE[n, {k}] or [n * {k}], got shape {tuple(records.shape)}")
            count = records.size
        else:
            count = int(records.shape[0]) if hasattr(records, "data_ptr") and records.dim() == 2 else 0  # (_query_into refuses what is no tensor [n, 12])
        if count % k:
            raise NativeError(ERR_INVALID, f"box_overlaps_into: {count} records are not a multiple of k={k}: a box takes a group of {k} records")
        return self._query_into(records, fmt, BOX_OVERLAP_DTYPE, "box_overlaps_into", "BOX_OVERLAP_DTYPE")

    def sweep_spheres(self, org, dir, radius, tmax=math.inf) -> np.ndarray:
        """When and where the spheres of radius `radius` whose centres move along org[n, 3] + t dir[n, 3], t in [0, tmax], first touch the uploaded mesh —
        include/rvpt_hip.h: SPHERE SWEEPS has the definition, the arithmetic and the numbering of prim.  radius and tmax are scalars or one value per sphere;
        dir need not be unit (t is in its units), and dir = 0 asks whether the sphere overlaps the mesh where it stands.  Returns SPHERE_SWEEP_DTYPE[n]: t, prim,
        and the pair (u, v) of the point of that triangle nearest to the centre at t, which Context.surface_points turns into the contact point and the stored
        normal; prim == NO_PRIM (and t = tmax) where nothing is touched or the record is invalid."""
        org = np.asarray(org, dtype=np.float32)
        dirv = np.asarray(dir, dtype=np.float32)
        if org.ndim == 0 or org.size % 3 or org.shape != dirv.shape or (org.ndim > 1 and org.shape[-1] != 3):
            raise NativeError(ERR_INVALID, f"sweep_spheres: org[n, 3] and dir[n, 3] are needed, got shapes {tuple(org.shape)} and {tuple(dirv.shape)}")
        org, dirv = org.reshape(-1, 3), dirv.reshape(-1, 3)
        rec = np.zeros(org.shape[0], dtype=SPHERE_SWEEP_DTYPE)
        rec["org"], rec["dir"] = org, dirv
        for name, value in (("radius", radius), ("tmax", tmax)):
            value = np.asarray(value, dtype=np.float32)
            if value.ndim > 1 or (value.ndim == 1 and value.shape[0] != org.shape[0]):
                raise NativeError(ERR_INVALID, f"sweep_spheres: {org.shape[0]} spheres, {name} of shape {tuple(value.shape)}")
            rec[name] = value
        return self.sweep_spheres_into(rec)

    def sweep_spheres_into(self, records):
        """rvpt_hip_read with FORMAT_SPHERE_SWEEPS in the caller's memory: `records` is a contiguous SPHERE_SWEEP_DTYPE array, or a contiguous float32 torch
        tensor [n, 12] (48-byte records; prim is the bits of its float) on the host or on this context's device, as for trace_rays_into.  The in quads (org,
        radius, dir, tmax) stay as they are, the out quad is written.  Returns records."""
        return self._query_into(records, FORMAT_SPHERE_SWEEPS, SPHERE_SWEEP_DTYPE, "sweep_spheres_into", "SPHERE_SWEEP_DTYPE")

    def read_triangles(self) -> np.ndarray:
        """rvpt_hip_read with FORMAT_TRIANGLES: the stored triangle rows as the last update form left them — all 64 bytes of each, nothing recomputed — as
        float32[n, 16] in the order update_triangles takes on this context (the leaf order after upload_scene, the caller's own after build_scene or a guarded
        rebuild).  include/rvpt_hip.h: TRIANGLES."""
        if self._scene_tris is None:
            _check(self._L.rvpt_hip_read(self._h, FORMAT_TRIANGLES, None, 0), self._h, self._L)  # (the library's own refusal: no scene)
        out = np.empty((int(self._scene_tris or 0), 16), dtype=np.float32)
        _check(self._L.rvpt_hip_read(self._h, FORMAT_TRIANGLES, _ptr(out) if out.size else None, out.nbytes), self._h, self._L)
        return out

    def read_triangles_into(self, dst):
        """read_triangles into the caller's memory: `dst` is a contiguous float32[n, 16] numpy array, or a contiguous float32 torch tensor [n, 16] on the host or
        on this context's device — the rows then never visit the host.  More rows than the scene holds are allowed; those past the scene's are not touched.
        On return the library's stream has finished writing.  Returns dst."""
        is_tensor = not isinstance(dst, np.ndarray) and hasattr(dst, "data_ptr")
        if is_tensor:
            import torch
            if dst.dtype != torch.float32 or dst.dim() != 2 or dst.shape[1] != 16 or not dst.is_contiguous():
                raise NativeError(ERR_INVALID, f"read_triangles_into: a contiguous float32 tensor [n, 16] is needed, got {dst.dtype} {tuple(dst.shape)}")
            nbytes = int(dst.shape[0]) * 64
            if dst.is_cuda:
                if dst.device.index != self.device:
                    raise NativeError(ERR_INVALID, f"read_triangles_into: the tensor lives on device {dst.device.index}, the context on {self.device}")
                torch.cuda.current_stream(dst.device).synchronize()  # the library works on its own stream: what touched the tensor last must have finished
                ptr = C.c_void_p(dst.data_ptr())
            else:
                ptr = _ptr(dst.numpy())  # (shares the tensor's memory)
        elif isinstance(dst, np.ndarray):
            if dst.dtype != np.float32 or dst.ndim != 2 or dst.shape[1] != 16 or not dst.flags.c_contiguous or not dst.flags.writeable:
                raise NativeError(ERR_INVALID, f"read_triangles_into: a contiguous writeable float32[n, 16] array is needed, got {dst.dtype} {tuple(dst.shape)}")
            ptr, nbytes = _ptr(dst), dst.nbytes
        else:
            raise NativeError(ERR_INVALID, f"read_triangles_into: a numpy array or a torch tensor is needed, got {type(dst).__name__}")
        _check(self._L.rvpt_hip_read(self._h, FORMAT_TRIANGLES, ptr if nbytes else None, nbytes), self._h, self._L)
        return dst

    def surface_points(self, prim, u, v) -> np.ndarray:
        """Points on the stored mesh, as the last update form left it, for the (prim, u, v) a query reported — include/rvpt_hip.h: SURFACE POINTS has the
        convention (u weights vert1 - vert0, v weights vert2 - vert0), the arithmetic and the numbering of prim (a ray query's).  prim[n] unsigned, u[n], v[n]
        float32.  Returns SURFACE_POINT_DTYPE[n]: point, mat, normal; an invalid record (prim outside the scene — NO_PRIM, a miss piped through —, a non-finite
        u or v) goes out as point = normal = 0, mat = NO_PRIM."""
        prim = np.asarray(prim)
        if prim.dtype.kind not in "iu" or (prim.size and (prim.min() < 0 or prim.max() > 0xFFFFFFFF)):
            raise NativeError(ERR_INVALID, f"surface_points: prim must be integers in [0, 2^32), got {prim.dtype}")
        prim = prim.astype(np.uint32).reshape(-1)
        uv = [np.asarray(x, dtype=np.float32) for x in (u, v)]
        for name, x in zip("uv", uv):
            if x.ndim > 1 or (x.ndim == 1 and x.shape[0] != prim.shape[0]):
                raise NativeError(ERR_INVALID, f"surface_points: {prim.shape[0]} records, {name} of shape {tuple(x.shape)}")
        rec = np.zeros(prim.shape[0], dtype=SURFACE_POINT_DTYPE)
        rec["prim"], rec["u"], rec["v"] = prim, uv[0], uv[1]
        return self.surface_points_into(rec)

    def surface_points_into(self, records):
        """rvpt_hip_read with FORMAT_SURFACE_POINTS in the caller's memory: `records` is a contiguous SURFACE_POINT_DTYPE array, or a contiguous float32 torch
        tensor [n, 12] (48-byte records; prim, flags, mat and reserved are the bits of their floats) on the host or on this context's device, as for
        trace_rays_into.  The in fields (prim, u, v, flags) stay as they are, the out fields are written.  Returns records."""
        return self._query_into(records, FORMAT_SURFACE_POINTS, SURFACE_POINT_DTYPE, "surface_points_into", "SURFACE_POINT_DTYPE")

    def write_accum(self, img) -> None:
        """rvpt_hip_write_accum: restore the accumulator from a row-major RGBA32F frame — anything numpy makes float32[h, w, 4] of, or a contiguous float32
        torch tensor [h, w, 4] on this context's device, which the tiling kernel reads in place."""
        if not isinstance(img, np.ndarray) and hasattr(img, "data_ptr") and img.is_cuda:  # (a tensor in host memory goes the way it always went: through numpy)
            ptr, nbytes, keep = self._frame_buffer(img, FORMAT_RGBA32F, "write_accum")
            _check(self._L.rvpt_hip_write_accum(self._h, ptr, nbytes), self._h, self._L)
            del keep
            return
        img = np.ascontiguousarray(img, dtype=np.float32).reshape(self.height, self.width, 4)
        _check(self._L.rvpt_hip_write_accum(self._h, _ptr(img), img.nbytes), self._h, self._L)

    def tile_buffer(self):
        """(device_ptr, bytes, max_tile_bytes) of this rank's tile-linear accumulator."""
        p, b, m = C.c_void_p(None), C.c_size_t(0), C.c_size_t(0)
        _check(self._L.rvpt_hip_tile_buffer(self._h, C.byref(p), C.byref(b), C.byref(m)), self._h, self._L)
        return p.value, b.value, m.value

    def comm_init(self, unique_id: bytes) -> None:
        """rvpt_hip_comm_init: join the RCCL communicator of this image's tile_world ranks (rank = tile_rank)."""
        _check(self._L.rvpt_hip_comm_init(self._h, unique_id, len(unique_id)), self._h, self._L)

    def comm_info(self):
        """rvpt_hip_comm_info: (ranks, this rank, RCCL version) as RCCL itself reports them for the context's communicator."""
        n, r, v = C.c_int(0), C.c_int(-1), C.c_int(0)
        _check(self._L.rvpt_hip_comm_info(self._h, C.byref(n), C.byref(r), C.byref(v)), self._h, self._L)
        return n.value, r.value, v.value

    def comm_destroy(self) -> None:
        """rvpt_hip_comm_destroy: leave the communicator (reads become local again)."""
        _check(self._L.rvpt_hip_comm_destroy(self._h), self._h, self._L)

    def comm_barrier(self) -> None:
        """rvpt_hip_comm_barrier (collective): this rank's work has finished, then a one-float all-reduce on the communicator."""
        _check(self._L.rvpt_hip_comm_barrier(self._h), self._h, self._L)

    def gather(self, dst_ptr) -> None:
        """rvpt_hip_gather (collective): rank 0 passes a device pointer to width*height*16 bytes, the others None."""
        _check(self._L.rvpt_hip_gather(self._h, C.c_void_p(dst_ptr) if dst_ptr else None), self._h, self._L)

    def untile(self, gathered_ptr: int, slot_bytes: int, n_ranks: int, dst_ptr: int) -> None:
        _check(self._L.rvpt_hip_untile(self._h, C.c_void_p(gathered_ptr), slot_bytes, n_ranks, C.c_void_p(dst_ptr)), self._h, self._L)

    def timing(self):
        """(last_ms, sum_ms, n_dispatches) of the frame kernel (needs the TIMING flag)."""
        last, tot, n = C.c_float(0), C.c_double(0), C.c_uint64(0)
        _check(self._L.rvpt_hip_get_timing(self._h, C.byref(last), C.byref(tot), C.byref(n)), self._h, self._L)
        return last.value, tot.value, n.value

    def reset_timing(self) -> None:
        _check(self._L.rvpt_hip_reset_timing(self._h), self._h, self._L)

    def launch_info(self):
        """(work-groups, LDS bytes per work-group, kernel variant, frames in flight) of the last dispatch."""
        g, l, v, f = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(self._L.rvpt_hip_get_launch_info(self._h, C.byref(g), C.byref(l), C.byref(v), C.byref(f)), self._h, self._L)
        return g.value, l.value, v.value, f.value

    def cull_info(self) -> int:
        """rvpt_hip_get_cull_info of the last launch: bit 0 screen rectangles, bit 1 bounce table, bit 2 camera rounds aligned to 16 x 4 blocks, bit 4 leaf boxes,
        bit 5 interleaved claim order, bit 6 the kernel instance without the uncull'd walks, bit 7 (CULL_SKY_LIST) the batched launch that claims only the blocks
        that are not sky and blends the sky from the RNG, bit 8 (CULL_ROW_BOXES) the row boxes of bounce packets that leave one triangle, bit 9 (CULL_FRAME_RUNS) the listed launch in frame-run order,
        bit 10 (CULL_ROW_RULE_TIGHT) those row boxes were made by the tight rule (the laboratory build's RVPT_HIP_PACKETS_ROW_RULE=0 at upload_scene: round 8's)."""
        f = C.c_uint32(0)
        _check(self._L.rvpt_hip_get_cull_info(self._h, C.byref(f)), self._h, self._L)
        return f.value

    def selftest_camera_rects(self, n_samples: int = 1, n_tris: int = 0):
        """rvpt_hip_selftest_camera_rects on this context's scene / camera / image size.  Returns (counts, prepared, rects): counts = (accepted pairs,
        accepted pairs outside their rectangle — the claim is 0 —, (block, triangle) pairs whose rectangle holds the block, all such pairs); with
        n_tris > 0 also the device's prepared records float32[n_tris, 16] and rectangles int32[n_tris, 4]."""
        out = (C.c_uint64 * 4)()
        prep = np.zeros((n_tris, 16), dtype=np.float32) if n_tris else None
        rects = np.zeros((n_tris, 2), dtype=np.uint32) if n_tris else None
        _check(self._L.rvpt_hip_selftest_camera_rects(self._h, int(n_samples), out, _ptr(prep), _ptr(rects)), self._h, self._L)
        return tuple(int(x) for x in out), prep, (unpack_rects(rects) if n_tris else None)

    def selftest_bounce_cull(self, n_samples: int = 1):
        """rvpt_hip_selftest_bounce_cull: (accepted pairs on segments that leave a triangle, those the bounce cull's table excludes — the claim is 0 —, bits set in
        the table, bits in the table, accepted pairs whose ray fails its triangle's leaf box — the claim is 0 —, (segment, leaf box) pairs tested, passed, accepted pairs
        that the refined row or the row box of where the segment leaves from excludes — the claim is 0)."""
        out = (C.c_uint64 * 8)()
        _check(self._L.rvpt_hip_selftest_bounce_cull(self._h, int(n_samples), out), self._h, self._L)
        return tuple(int(x) for x in out)

    def scene_state(self, pieces=None) -> dict:
        """rvpt_hip_selftest_scene_state (laboratory contexts only): the stored scene as the device holds it, after everything queued has finished.  Returns a dict
        with the info block's fields (n_tris, n_nodes, n_wide, bvh_head_shift, wide_stack_levels, bvh_height, built_by as None / "lbvh" / "ploc" / "sah", the
        have_* flags as bools, base_cost) and, per name of SCENE_STATE_PIECES (all of them, or those listed in `pieces`), a numpy array of exactly the live bytes
        — empty where the context does not hold the piece now.  Nothing is launched and nothing changes."""
        if not self.lab:
            raise NativeError(ERR_UNSUPPORTED, "scene_state: only the laboratory build reads the scene back (Context(..., lab=True))")
        info, size = SceneStateInfo(), C.c_size_t(0)
        _check(self._L.rvpt_hip_selftest_scene_state(self._h, C.byref(info), 0, None, 0, C.byref(size)), self._h, self._L)
        out = {name: getattr(info, name) for name, _ in SceneStateInfo._fields_}
        for flag in ("have_perm", "have_sparse_maps", "have_inv_perm", "have_cost"):
            out[flag] = bool(out[flag])
        out["built_by"] = BUILT_BY[info.built_by]
        for name in (SCENE_STATE_PIECES if pieces is None else pieces):
            number, dtype, tail = SCENE_STATE_PIECES[name]
            rc = self._L.rvpt_hip_selftest_scene_state(self._h, None, number, None, 0, C.byref(size))
            if rc not in (0, ERR_SIZE):
                _check(rc, self._h, self._L)
            item = np.dtype(dtype).itemsize * int(np.prod(tail, dtype=np.int64))
            buf = np.zeros((size.value // item,) + tail, dtype=dtype)
            if size.value:
                assert buf.nbytes == size.value, (name, buf.nbytes, size.value)
                _check(self._L.rvpt_hip_selftest_scene_state(self._h, None, number, _ptr(buf), buf.nbytes, C.byref(size)), self._h, self._L)
            out[name] = buf
        return out

    def stats(self):
        """(segments, samples) traced since create / reset_timing (needs COUNT_SEGMENTS)."""
        s = (C.c_uint64 * 2)()
        _check(self._L.rvpt_hip_get_stats(self._h, s), self._h, self._L)
        return int(s[0]), int(s[1])
