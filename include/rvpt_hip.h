/*
 * rvpt_hip.h — C ABI of the MI355X (gfx950) path-trace backend that replaces RVPT's
 * VkComputePipeline dispatch of assets/shaders/compute_pass.comp.
 *
 * The reference has no plugin/FFI layer; the seam sits inside `class RVPT`
 * (src/rvpt/rvpt.{h,cpp}).  Every entry point below names the reference code it
 * replaces (paths relative to the reference tree).  Plain pointers and sizes only;
 * no exceptions, asserts or C++/torch types cross this boundary.
 *
 * All functions return 0 on success and a negative RVPT_HIP_ERR_* code on failure;
 * rvpt_hip_last_error() gives the text (mirrors VK_CHECK_RESULT + fmt::print,
 * src/rvpt/vk_util.h:18-27).
 *
 * One context == one GPU == one process rank.  A context is not thread-safe (the
 * reference is single-threaded; Queue::submit_mutex, src/rvpt/vk_util.h:160, is
 * never contended).  The caller owns every host array; the library owns all device
 * memory and keeps no host pointer after a call returns.
 *
 * PROCESS ENVIRONMENT: the library never modifies it.  A context creates seven HIP streams of its own (six
 * for launches in flight — three rotate for most launches, six for short BVH launches — plus one for
 * uploads, the temporal blend and read-back); ROCm maps streams onto GPU_MAX_HW_QUEUES hardware queues
 * (default 4), so a host that wants the published throughput sets GPU_MAX_HW_QUEUES=8 (or more) BEFORE the
 * first HIP call of the process (measured: -10 % when two frame streams share a queue).  rvpt_hip_create
 * writes one line to stderr, once per process, when it finds the variable unset or below 8
 * (RVPT_HIP_QUIET=1 silences it).  INTEGRATION.md.
 */
#ifndef RVPT_HIP_H
#define RVPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVPT_HIP_ABI_VERSION 8 /* 2: + rvpt_hip_dispatch_frames, RVPT_HIP_TRAVERSAL_BVH_ORDERED; 3: + the RCCL communicator (comm_*, gather, collective read), selftest_*;
                                  4: + rvpt_hip_comm_barrier, bounded collectives (RVPT_HIP_COMM_TIMEOUT_S);
                                  5: the wavefront pipelines of ABI 3-4 are retired (flags 0x40 / 0x80 / 0x100 are rejected), + RVPT_HIP_BVH_PER_LANE;
                                     unknown flag bits are an error;
                                  6: + rvpt_camera_rects, rvpt_hip_selftest_camera_rects (the screen rectangles of the packet kernel's camera rounds), rvpt_hip_selftest_bounce_cull;
                                  7: + rvpt_bvh_quant_form (the 64-byte quantised wide nodes, RVPT_HIP_BVH_QUANT=1);
                                  8: the release library exports the 30 entry points of THIS header only — what a caller of `class RVPT` needs; the
                                     selftests, the host-side forms of the device data (rvpt_camera_rects, rvpt_bounce_rows, rvpt_bvh_wide_form,
                                     rvpt_bvh_quant_form), the opt-in walks that measured slower (8-wide, quantised) and the tuning knobs live in the
                                     laboratory build librvpt_hip_debug.so (include/rvpt_hip_lab.h); + rvpt_hip_build_flags, rvpt_hip_get_cull_info,
                                     rvpt_hip_comm_info.  Still 8, no new symbol: rvpt_hip_upload_scene called with triangles but without nodes and without
                                     materials — until then always an error — is a GEOMETRY UPDATE (moved vertices, the tree refitted on the device).  Still 8,
                                     no new symbol: on a BVH context, no nodes and the count RVPT_HIP_NODES_BUILD — until then the "needs nodes" error —
                                     is the BUILD FORM (the library builds the tree on the device from the triangles alone).  Still 8, no new symbol: the
                                     count RVPT_HIP_NODES_BUILD_PLOC — until then the "needs nodes" error too — is the build form with a PLOC tree.  Still 8, no
                                     new symbol: the count RVPT_HIP_NODES_BUILD_SAH — until then the "needs nodes" error as well — is the build form with the
                                     binned-SAH tree of rvpt_bvh_build, made on the device.  Still 8, no new symbol: `dst` of rvpt_hip_read and
                                     `src_rgba32f` of rvpt_hip_write_accum may be DEVICE MEMORY of the context's GPU — until then undefined — and the frame
                                     then never visits the host.  Still 8, no new symbol: no nodes and a count RVPT_HIP_NODES_UPDATE_GUARDED(permille) — until then the
                                     "needs nodes" error — is the GUARDED UPDATE: the update form, the SAH cost of the refitted tree computed on the device and
                                     reported, and past a limit a rebuild by the builder that made the tree.  Still 8, no new symbol: the count
                                     RVPT_HIP_NODES_UPDATE_SPARSE with `nodes` pointing at a list of triangle indices — until then an error on brute-force
                                     contexts and a read past the list on BVH contexts — is the SPARSE UPDATE: the listed triangles move, only the boxes on
                                     their paths to the root are recomputed.  Still 8, no new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_RAY_HITS (2) —
                                     until then the "unknown format" error — is a RAY QUERY: `dst` holds rvpt_ray_hit records, rays in and hits out, in place.  Still 8, no
                                     new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_RAY_PATHS (3) — until then the "unknown format" error — is a
                                     PATH QUERY: `dst` holds rvpt_ray_path records, a ray, an RNG state and a bounce budget in, integrator_Kajiya's radiance out.  Still 8, no
                                     new symbol: the count RVPT_HIP_NODES_UPDATE_POSE with `nodes` pointing at a list of rvpt_part_move records — until then the
                                     "needs nodes" or "NULL scene array" error — is the POSE UPDATE: ranges of triangles move by one 3x4 matrix each, posed on
                                     the device from a rest pose it keeps, and only the boxes on their paths to the root are recomputed.  Still 8, no
                                     new symbol: the same arguments under a count RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) — until then the "NULL scene
                                     array" error — are the GUARDED POSE UPDATE: the pose update, the SAH cost of the posed tree reported, and past a limit a
                                     rebuild by the builder that made the tree, through which the rest pose follows its triangles.  Still 8, no
                                     new symbol: the count RVPT_HIP_NODES_BIND_SKIN with `nodes` pointing at three rvpt_vertex_skin records per stored
                                     triangle — until then the "NULL scene array" error — is the BIND: four bone indices and four weights per vertex, kept
                                     on the device.  Still 8, no new symbol: the count RVPT_HIP_NODES_UPDATE_SKIN with `nodes` pointing at a list of rvpt_bone
                                     matrices — until then the "NULL scene array" error — is the SKIN UPDATE: every vertex posed from the rest pose by its
                                     four weighted matrices (linear blend skinning), every box refitted.  Still 8, no
                                     new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_NEAREST_POINTS (4) — until then the "unknown format" error — is a
                                     POINT QUERY: `dst` holds rvpt_point_hit records, a point and a squared bound in, the nearest point of the mesh, its squared
                                     distance and its triangle out.  Still 8, no new symbol: rvpt_hip_read with a format RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode)
                                     (16 .. 25) — until then the "unknown format" error — is a PATH QUERY BY INTEGRATOR: the records of format 3, each
                                     evaluated by the render mode 0 .. 9 of compute_pass.comp the call names; mode 9 is format 3 itself.  Still 8, no new
                                     symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_TRIANGLES (5) — until then the "unknown format" error — is the
                                     TRIANGLE READ-BACK: `dst` receives the stored rvpt_triangle rows, as the last update form left them, in update order.
                                     Still 8, no new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_SURFACE_POINTS (6) — until then the "unknown
                                     format" error — is a SURFACE POINT read: `dst` holds rvpt_surface_point records, (prim, u, v) as a query reported them
                                     in, the point of the stored mesh, its material word and its normal out.  Still 8, no new symbol: rvpt_hip_read with
                                     a format RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k) (33 .. 40) — until then the "unknown format" error — is a K-NEAREST RAY
                                     QUERY: `dst` holds groups of k rvpt_ray_hit records, the ray in the first, the k nearest hits along it out.  Still 8, no
                                     new symbol: the skin update's arguments under a count RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille) — until then the
                                     "NULL scene array" error — are the GUARDED SKIN UPDATE: the skin update, the SAH cost of the skinned tree reported, and
                                     past a limit a rebuild by the builder that made the tree, through which the rest pose follows its triangles and the
                                     binding stays.  Still 8, no new symbol: rvpt_hip_read with a format RVPT_HIP_FORMAT_NEAREST_POINTS_K(k) (49 .. 56) —
                                     until then the "unknown format" error — is a K-NEAREST POINT QUERY: `dst` holds groups of k rvpt_point_hit records,
                                     the point in the first, the k nearest triangles of the mesh out.  Still 8, no new symbol: rvpt_hip_read with the
                                     format RVPT_HIP_FORMAT_RAY_CROSSINGS (8) — until then the "unknown format" error — is a CROSSING QUERY: `dst` holds
                                     rvpt_ray_crossings records, rays in, the counts of front and back hits along them and the first and last t out.
                                     Still 8, no new symbol: rvpt_hip_read with the format RVPT_HIP_FORMAT_BOX_OVERLAPS (9) or a format
                                     RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k) (65 .. 68) — until then the "unknown format" error — is a BOX QUERY: `dst` holds
                                     groups of k rvpt_box_overlap records, a closed box in the first, the count of the triangles that meet it and the
                                     smallest of their numbers out.  Still 8, no new symbol: rvpt_hip_read with the format
                                     RVPT_HIP_FORMAT_SPHERE_SWEEPS (10) — until then the "unknown format" error — is a SPHERE SWEEP: `dst` holds
                                     rvpt_sphere_sweep records, a sphere and the motion of its centre in, the time of its first contact with the mesh,
                                     the triangle and the barycentric pair out */

/* ---- POD layouts: byte-identical to the reference's GPU buffers ------------------ */

/* src/rvpt/geometry.h:76-111 == assets/shaders/structs.glsl:1-7 (64 B).
 * vert{0,1,2}[3] hold the host-side face normal (unused by the live shader code);
 * mat_id[0] is the material index stored as a float. */
typedef struct rvpt_triangle {
    float vert0[4];
    float vert1[4];
    float vert2[4];
    float mat_id[4];
} rvpt_triangle;

/* src/rvpt/bvh.h:12-19 == structs.glsl:9-14 (32 B).  Root is node 0, the two children of
 * an inner node are `first` and `first+1`, a node is a leaf iff primitive_count > 0.
 * bounds = {minx,maxx,miny,maxy,minz,maxz} (assets/shaders/intersection.glsl:376-377). */
typedef struct rvpt_bvh_node {
    uint32_t first_child_or_primitive;
    uint32_t primitive_count;
    float bounds[6];
} rvpt_bvh_node;

/* src/rvpt/material.h:9-26 == structs.glsl:22-33 (48 B).  type = (int)data[0]
 * (0 Lambert, 1 mirror, 2 dielectric); ior is read from albedo[3]
 * (assets/shaders/intersection.glsl:45-57). */
typedef struct rvpt_material {
    float albedo[4];
    float emission[4];
    float data[4];
} rvpt_material;

/* src/rvpt/rvpt.h:77-89 == compute_pass.comp:28-40 (std140, 40 B). */
typedef struct rvpt_render_settings {
    int32_t max_bounces;
    int32_t aa;
    uint32_t current_frame;
    int32_t camera_mode;
    int32_t top_left_render_mode;
    int32_t top_right_render_mode;
    int32_t bottom_left_render_mode;
    int32_t bottom_right_render_mode;
    float split_ratio[2];
} rvpt_render_settings;

/* Camera::get_data(), src/rvpt/camera.cpp:55-66 == compute_pass.comp:44-49 (80 B):
 * column-major camera-to-world mat4, then params = (aspect, vfov_rad, ortho_scale, 0). */
typedef struct rvpt_camera_data {
    float matrix[16];
    float params[4];
} rvpt_camera_data;

/* ---- error codes ------------------------------------------------------------------ */
#define RVPT_HIP_OK 0
#define RVPT_HIP_ERR_INVALID (-1)     /* bad argument / call order                       */
#define RVPT_HIP_ERR_HIP (-2)         /* a HIP runtime call failed                       */
#define RVPT_HIP_ERR_UNSUPPORTED (-3) /* reserved: every render / camera mode of compute_pass.comp is implemented */
#define RVPT_HIP_ERR_NO_DEVICE (-4)   /* no gfx950 device visible                        */
#define RVPT_HIP_ERR_SIZE (-5)        /* destination buffer too small                    */
#define RVPT_HIP_ERR_COMM (-6)        /* RCCL missing or a collective call failed        */

/* ---- create flags ------------------------------------------------------------------- */
#define RVPT_HIP_TRAVERSAL_BRUTE 0x0u /* LDS-staged brute-force closest hit (north star)  */
#define RVPT_HIP_TRAVERSAL_BVH 0x1u   /* intersect_bvh semantics (intersection.glsl:361)  */
#define RVPT_HIP_TRAVERSAL_BVH_ORDERED 0x2u /* same BVH, nearer child first — the reference's own
                                         "TODO: Order the children on the stack" (intersection.glsl:405); same image
                                         except where exact ties / slab rounding decide, far fewer nodes visited */
#define RVPT_HIP_TRAVERSAL_MASK 0x3u
#define RVPT_HIP_COUNT_SEGMENTS 0x4u  /* count path segments (for the roofline model)     */
#define RVPT_HIP_KERNEL_SIMPLE 0x8u   /* one-pixel-per-lane kernel, no ray regeneration   */
#define RVPT_HIP_TIMING 0x10u         /* bracket every frame kernel with hipEvents        */
#define RVPT_HIP_ACCUM_UNORM8 0x20u   /* reference-format accumulation: the running mean is clamped to [0,1]
                                         and rounded to 8 bits after every frame, as storing to the rgba8
                                         temporal image does (compute_pass.comp:41-42,165); default is FP32 */
#define RVPT_HIP_BRUTE_MIXED_PACKETS 0x200u /* brute-force contexts: round 2's frame kernel (a lane takes its next pixel the moment its pixel
                                          is finished: packets mix camera and bounce rays) instead of the packet kernel that is the default
                                          for LDS-resident scenes in the lean configuration (rvpt_packets.hip: full packets of one kind per
                                          round, camera rays with the packet-uniform early-out).  Same image either way */
#define RVPT_HIP_BVH_PER_LANE 0x400u  /* BVH contexts: rounds 1-3's kernels — binary nodes, every segment walks the tree per lane — instead of the walk over the
                                         4-wide regrouping of the tree (rvpt_bvh4.hip; with camera packets where the scene is LDS-resident) that is the default
                                         for the reference's child order.  Same image */
#define RVPT_HIP_FLAGS_KNOWN 0x63Fu   /* every bit above; rvpt_hip_create rejects anything else (0x40, 0x80, 0x100: the wavefront
                                         pipelines of ABI 3-4, measured at 0.55x / 0.7x of the persistent kernels and retired) */

/* ---- read formats --------------------------------------------------------------------- */
#define RVPT_HIP_FORMAT_RGBA32F 0     /* float radiance running mean, alpha 0            */
#define RVPT_HIP_FORMAT_RGBA8_UNORM 1 /* clamp+quantise of the above (reference image format,
                                         compute_pass.comp:41-42)                        */
#define RVPT_HIP_FORMAT_RAY_HITS 2    /* dst: rvpt_ray_hit[dst_bytes / 48], in and out (RAY QUERIES at rvpt_hip_read) */
#define RVPT_HIP_RAY_ANY_HIT 0x1u     /* per ray: stop at the first accepted triangle    */
#define RVPT_HIP_RAY_MAX_HITS 8u      /* per call: the largest k of a k-nearest ray query */
#define RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k) (32 + (k))     /* k = 1 .. RVPT_HIP_RAY_MAX_HITS: formats 33 .. 40; dst: n groups of k rvpt_ray_hit (K-NEAREST RAY QUERIES at rvpt_hip_read) */

/* One ray of a query and its answer (48 B = three float4; no reference counterpart: the reference traces only its camera's paths). */
typedef struct rvpt_ray_hit {
    float org[3]; float tmax;        /* in: the interval is (0, tmax); +inf = the reference's */
    float dir[3]; uint32_t flags;    /* in: 0 or RVPT_HIP_RAY_ANY_HIT; other bits reserved, ignored */
    float t; uint32_t prim; float u; float v;   /* out */
} rvpt_ray_hit;

#define RVPT_HIP_FORMAT_RAY_CROSSINGS 8  /* dst: rvpt_ray_crossings[dst_bytes / 48], in and out (RAY CROSSINGS at rvpt_hip_read) */

/* One ray of a crossing query and its answer (48 B = three float4; the first two quads are an rvpt_ray_hit's). */
typedef struct rvpt_ray_crossings {
    float org[3]; float tmax;        /* in: as rvpt_ray_hit */
    float dir[3]; uint32_t flags;    /* in: reserved, ignored — RVPT_HIP_RAY_ANY_HIT included */
    uint32_t front; uint32_t back; float t_near; float t_far;   /* out */
} rvpt_ray_crossings;

#define RVPT_HIP_FORMAT_RAY_PATHS 3   /* dst: rvpt_ray_path[dst_bytes / 48], in and out (PATH QUERIES at rvpt_hip_read) */
#define RVPT_HIP_PATH_MAX_BOUNCES 1024u /* per path: the largest bounce budget a record may ask for */
#define RVPT_HIP_FORMAT_RAY_PATHS_MODE(mode) (16 + (mode))   /* mode 0 .. 9: the render modes of compute_pass.comp:76-95 */

/* One path of a query and its answer (48 B = three float4; no reference counterpart: the reference traces only its camera's paths). */
typedef struct rvpt_ray_path {
    float org[3]; uint32_t seed;          /* in: the first segment's origin; the RNG state the path starts from */
    float dir[3]; uint32_t max_bounces;   /* in: the first segment's direction (need not be unit); the bounce budget, 1 .. RVPT_HIP_PATH_MAX_BOUNCES */
    float radiance[3]; uint32_t segments; /* out */
} rvpt_ray_path;

#define RVPT_HIP_FORMAT_NEAREST_POINTS 4 /* dst: rvpt_point_hit[dst_bytes / 48], in and out (NEAREST POINTS at rvpt_hip_read) */

/* One point of a query and its answer (48 B = three float4; no reference counterpart: the reference asks its scene nothing but its camera's paths). */
typedef struct rvpt_point_hit {
    float point[3];   float max_d2;                        /* in: the query point; the search bound as a SQUARED distance, +inf = unbounded */
    float closest[3]; float d2;                            /* out: the nearest point of the mesh and its squared distance */
    uint32_t prim;    float u; float v; uint32_t region;   /* out: the triangle, the pair the region computed, 0 face, 1/2/3 vertex a/b/c, 4/5/6 edge ab/ac/bc */
} rvpt_point_hit;

#define RVPT_HIP_POINT_MAX_NEAREST 8u /* per call: the largest k of a k-nearest point query */
#define RVPT_HIP_FORMAT_NEAREST_POINTS_K(k) (48 + (k))     /* k = 1 .. RVPT_HIP_POINT_MAX_NEAREST: formats 49 .. 56; dst: n groups of k rvpt_point_hit (K-NEAREST POINTS at rvpt_hip_read) */

#define RVPT_HIP_FORMAT_BOX_OVERLAPS 9   /* dst: rvpt_box_overlap[dst_bytes / 48], in and out (BOX OVERLAPS at rvpt_hip_read) */

/* One box of a query and its answer (48 B = three float4; no reference counterpart: the reference asks its scene nothing but its camera's paths). */
typedef struct rvpt_box_overlap {
    float lo[3]; uint32_t prim_from;     /* in: the box is [lo, hi] per axis, closed; only triangles whose reported number is >= prim_from take part */
    float hi[3]; uint32_t flags;         /* in: flags reserved, ignored */
    uint32_t count; uint32_t prim[3];    /* out: how many triangles meet the box; the smallest of their numbers, ascending, 0xFFFFFFFF past the last */
} rvpt_box_overlap;

#define RVPT_HIP_BOX_MAX_GROUP 4u /* per call: the largest k of a box query's groups */
#define RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k) (64 + (k))       /* k = 1 .. RVPT_HIP_BOX_MAX_GROUP: formats 65 .. 68; dst: n groups of k rvpt_box_overlap listing 4k - 1 numbers (BOX OVERLAPS at rvpt_hip_read) */

#define RVPT_HIP_FORMAT_SPHERE_SWEEPS 10 /* dst: rvpt_sphere_sweep[dst_bytes / 48], in and out (SPHERE SWEEPS at rvpt_hip_read) */

/* One moving sphere of a query and its first contact (48 B = three float4; no reference counterpart: the reference asks its scene nothing but its camera's paths). */
typedef struct rvpt_sphere_sweep {
    float org[3]; float radius;                 /* in: the centre at t = 0; radius >= 0 */
    float dir[3]; float tmax;                   /* in: the centre is org + t*dir, t in [0, tmax] (closed; +inf allowed); dir need not be unit */
    float t; uint32_t prim; float u; float v;   /* out: laid out as the out quad of an rvpt_ray_hit */
} rvpt_sphere_sweep;

#define RVPT_HIP_FORMAT_TRIANGLES 5      /* dst: rvpt_triangle[n_tris], out: the stored rows in update order (TRIANGLES at rvpt_hip_read) */
#define RVPT_HIP_FORMAT_SURFACE_POINTS 6 /* dst: rvpt_surface_point[dst_bytes / 48], in and out (SURFACE POINTS at rvpt_hip_read) */

/* One point on the stored mesh (48 B = three float4; no reference counterpart).  The first quad is laid out as the last quad of an rvpt_point_hit. */
typedef struct rvpt_surface_point {
    uint32_t prim; float u; float v; uint32_t flags;   /* in: a triangle in the queries' numbering, the pair a query reported; flags reserved, ignored */
    float point[3];  uint32_t mat;                     /* out: (a + (b-a)*u) + (c-a)*v of the stored row, its material word */
    float normal[3]; uint32_t reserved;                /* out: the stored unit normal; reserved is written 0 */
} rvpt_surface_point;

/* Image tiles are RVPT_HIP_TILE x RVPT_HIP_TILE pixels — the footprint of one reference
 * work-group (compute_pass.comp:27).  The tile at (tx, ty) of the tiles_x-wide tile grid has slot
 * s = ty * tiles_x + (tx + RVPT_HIP_TILE_SHIFT * ty) % tiles_x (row-major, every row rotated by
 * RVPT_HIP_TILE_SHIFT more tiles than the one above: a diagonal pattern even where tiles_x is a
 * multiple of tile_world) and is owned by rank s % tile_world as that rank's local tile s / tile_world
 * (ABI 5; ABI <= 4: s = ty * tiles_x + tx, which gave each of 8 ranks whole tile columns of a 1920-wide image). */
#define RVPT_HIP_TILE 16
#define RVPT_HIP_TILE_SHIFT 3

typedef struct rvpt_hip_ctx rvpt_hip_ctx;

int rvpt_hip_abi_version(void);
/* (ABI 8) What this build of the library carries: RVPT_HIP_BUILD_LAB = the laboratory build (include/rvpt_hip_lab.h), RVPT_HIP_BUILD_DEBUG_CHECKS = the
 * kernels' internal checks (a BVH traversal that pushes past the stack the host sized is reported by rvpt_hip_wait under RVPT_HIP_DEBUG=1; without them
 * rvpt_hip_create refuses RVPT_HIP_DEBUG=1 instead of ignoring it). */
#define RVPT_HIP_BUILD_LAB 0x1u
#define RVPT_HIP_BUILD_DEBUG_CHECKS 0x2u
uint32_t rvpt_hip_build_flags(void);

/* Number of usable devices (replaces vk-bootstrap device selection, rvpt.cpp:477-570). */
int rvpt_hip_device_count(int *count);

/* Replaces create_rendering_resources()/add_per_frame_data(): pipeline (rvpt.cpp:676-681),
 * temporal image (rvpt.cpp:759-766), per-frame buffers + output image (rvpt.cpp:798-866).
 * Allocates the scene buffers and this rank's RGBA32F accumulator tiles on `device_id`.
 * tile_rank/tile_world select the image partition (1 GPU: 0/1). */
int rvpt_hip_create(rvpt_hip_ctx **out, int device_id, uint32_t width, uint32_t height,
                    uint32_t tile_rank, uint32_t tile_world, uint32_t flags);
void rvpt_hip_destroy(rvpt_hip_ctx *ctx);

/* Replaces the three scene memcpys the reference repeats every frame (rvpt.cpp:124-126).
 * Call when the scene changes.  `nodes` may be NULL for brute-force contexts.  Triangles must
 * already be in BVH-leaf order (Bvh::permute_primitives, bvh.h:72-79) for BVH contexts.
 *
 * GEOMETRY UPDATE — the form for a mesh whose vertices move while its topology stays (what the reference's
 * per-frame triangle copy, rvpt.cpp:124, is for):
 *
 *     rvpt_hip_upload_scene(ctx, NULL, 0, tris, n_tris, NULL, 0);      n_tris > 0
 *
 * - Legal only after a successful full upload on this context and only with the same n_tris; otherwise
 *   RVPT_HIP_ERR_INVALID, rvpt_hip_last_error says which, and the stored scene is untouched.  (Without triangles
 *   the call is what it always was: a full upload of the empty scene.)
 * - Only the twelve floats vert0..vert2 of every triangle are taken, in the leaf order of the full upload.  The
 *   stored mat_id rows, the materials and the topology of the tree (every node's first / count words) are kept.
 * - Every box of the tree is REFITTED on the device: a leaf's box becomes the component-wise min / max over the
 *   vertices of its triangles, an inner node's box the min / max of its two children's boxes.  min / max of
 *   floats is exact, so this is the same tree a host refit gives (rvpt_amd/scene.py: refit_bvh), and the context
 *   renders exactly what a full upload of (refitted nodes, tris, mats) would: images, statistics and tile buffers
 *   are bit-identical.  A caller's tree with LOOSE boxes therefore becomes TIGHT at the first update, even one
 *   that moves nothing.  A refit keeps the tree valid, not good: after large deformations a rebuilt tree
 *   traverses faster (DESIGN.md has the measurement) — rebuild and upload in full now and then.
 * - Frames in flight finish on the old geometry; `tris` may be freed on return; the accumulate / reset rule stays
 *   with the caller as for any scene change (set current_frame = 0).  Non-finite vertices are the caller's problem.
 * - On BVH contexts `tris` may also be DEVICE memory of the context's GPU (a buffer a simulation or a torch
 *   tensor lives in): the vertices then never visit the host.  The caller makes sure that whatever wrote the
 *   buffer has finished.  Brute-force contexts compute their scene scale and leaf boxes on the host: a device
 *   pointer there is RVPT_HIP_ERR_INVALID.
 * Cost, 1 M triangles: about the 48 MB host-to-device copy; rvpt_bvh_build + a full upload is two orders of
 * magnitude more.
 *
 * BUILD FORM — the library builds the tree, on the device, from the triangles alone:
 *
 *     rvpt_hip_upload_scene(ctx, NULL, RVPT_HIP_NODES_BUILD, tris, n_tris, mats, n_mats);
 *
 * - BVH contexts: a full upload whose tree is an LBVH made on the GPU (30-bit Morton codes of the centroids, a radix
 *   sort, leaves of at most two triangles; rvpt_amd/csrc/rvpt_build.h holds the definition, rvpt_amd/scene.py:
 *   build_lbvh is the same tree in numpy).  Brute-force contexts ignore nodes and n_nodes as they always have: there
 *   the call is the ordinary upload.  n_tris == 0 is the empty scene.
 * - `tris` arrive in the CALLER'S order, any order.  The library sorts its own copy and keeps the permutation.
 * - On BVH contexts `tris` may be device memory of the context's GPU, as in the update form; the material indices
 *   are then validated by a kernel.  A bad index is RVPT_HIP_ERR_INVALID naming the first offending triangle and
 *   leaves the stored scene untouched, for host and device sources alike.
 * - A second build-form call is a rebuild.  Frames in flight finish on the old scene.
 * - Only a bad material index is atomic.  Any other failure of a build (a HIP error, an allocation that fails, a tree
 *   higher than the traversal stack — which the definition rules out below 2^30 triangles) leaves the context WITHOUT a
 *   scene: the next call must be a full upload or another build form.
 * - The UPDATE FORM after a build form takes the triangles in that same caller's order (the vertex rows are gathered
 *   through the stored permutation); after an ordinary full upload it takes the leaf order of that upload, as above.
 * An LBVH is quick to build and traverses slower than the binned-SAH tree of rvpt_bvh_build: measured on one MI355X
 * (profiles/device_build.txt), 1 M triangles build in 4.5 ms from a host array and 1.8 ms from device memory against
 * 338 ms for rvpt_bvh_build + a full upload, and one-frame launches at 1080p run at 0.54 - 0.72 of the SAH tree's rate
 * — the number a caller chooses by (DESIGN.md 5.6 has the table and the frame counts at which a host build pays).
 *
 * BUILD FORM, PLOC TREE — the same call with the count RVPT_HIP_NODES_BUILD_PLOC:
 *
 *     rvpt_hip_upload_scene(ctx, NULL, RVPT_HIP_NODES_BUILD_PLOC, tris, n_tris, mats, n_mats);
 *
 * - The tree is made by parallel locally-ordered clustering (Meister & Bittner 2018) over the same sorted Morton order:
 *   bottom-up merging of nearest neighbours within 16 positions, leaves of one triangle (rvpt_amd/csrc/rvpt_build.h
 *   holds the definition, tie rule included; rvpt_amd/scene.py: build_ploc is the same tree in numpy).
 * - Everything said above holds: the caller's order, device pointers, the rebuild, the atomicity rule, the update
 *   form afterwards, brute-force contexts ignoring the count.  The two counts may alternate on one context.
 * - PLOC promises neither a height nor an iteration count.  A tree higher than 62 levels, or one not finished after
 *   256 iterations, is dropped and the call uploads the LBVH tree of RVPT_HIP_NODES_BUILD instead.  That is not an
 *   error: the call returns RVPT_HIP_OK, and rvpt_hip_last_error then holds a sentence that says so (after a PLOC tree
 *   it is empty).
 * By SAH cost the PLOC tree is at 0.65 - 0.84 of the LBVH's on the scenes of DESIGN.md 5.7; its build time and traversal
 * rate on an MI355X have not been measured yet (DESIGN.md 5.7 says what is open).
 *
 * BUILD FORM, SAH TREE — the same call with the count RVPT_HIP_NODES_BUILD_SAH:
 *
 *     rvpt_hip_upload_scene(ctx, NULL, RVPT_HIP_NODES_BUILD_SAH, tris, n_tris, mats, n_mats);
 *
 * - The tree is rvpt_bvh_build's: the top-down binned-SAH build (16 bins per axis over the centroid bounds, leaves of
 *   2 .. 8 triangles, median splits from depth 30 on) run level by level on the device.  Node for node the triangle
 *   sets and the boxes are those of rvpt_bvh_build; only the order of triangles inside a leaf may differ
 *   (rvpt_amd/csrc/rvpt_build.h: THE SAH TREE holds the definition with every tie rule; rvpt_amd/scene.py: build_sah
 *   is the same tree in numpy).  The traversal cost is 0: the device ignores RVPT_BVH_TRAVERSAL_COST.
 * - Everything said above holds: the caller's order, device pointers, the rebuild, the atomicity rule, the update
 *   form afterwards, brute-force contexts ignoring the count.  The three counts may alternate on one context.
 * - The height is at most 30 + ceil(log2 n) + 1 levels; there is no fallback.  rvpt_hip_last_error is empty after a
 *   SAH build.
 * DESIGN.md 5.8 has what was measured (profiles/device_build_sah.txt).
 *
 * GUARDED UPDATE — refit, cost the tree, rebuild when it has gone stale:
 *
 *     rvpt_hip_upload_scene(ctx, NULL, RVPT_HIP_NODES_UPDATE_GUARDED(permille), tris, n_tris, NULL, 0);      n_tris > 0
 *
 * permille is 0 (report only) or 1000 .. 65535: the limit as a factor of the base cost, in thousandths (1250 = 1.25).  Any other value, or materials passed
 * with this count, is RVPT_HIP_ERR_INVALID and leaves the stored scene untouched.
 * - BVH contexts.  Everything the update form says holds: the same n_tris, the order rule (the leaf order after an ordinary upload, the caller's order after a
 *   build form), host or device `tris`, frames in flight finishing on the old geometry, the stored scene untouched on a bad argument — with the update
 *   form's own messages.  Then:
 * - The TREE COST of the refitted tree is computed on the device and one double is read back.  Every binary node the root reaches is one term.  A node's
 *   extents are hi - lo per axis, taken in double from the float32 bounds; its half-area is ex*ey + ey*ez + ez*ex in double, in that order, every operation
 *   rounded on its own (no fused multiply-add).  An inner node contributes its half-area, a leaf its half-area times its primitive_count.  The sum
 *   is in double — a fixed order of additions, no atomics: the same tree gives the same 64 bits on every run — and is divided by the root's half-area.  A root
 *   of half-area 0 gives cost 0 and never triggers a rebuild.  rvpt_amd/scene.py: tree_cost is the same in numpy.
 * - The BASE COST is the cost of the tree that the last ordinary full upload or build form on this context left (recorded by every one of them on a BVH
 *   context: the same two kernels and one more 8-byte read).
 * - With a limit, if cost > (permille / 1000) * base cost and the stored scene came from a build form, the library REBUILDS with that build form's method
 *   (LBVH, PLOC with its fallback rule, SAH) from the moved vertices in the caller's order, the stored mat_id rows carried back through the stored
 *   permutation, and the materials as the caller last passed them.  What the context then holds — tree, permutation, level table, wide form, launch choice —
 *   is what rvpt_hip_upload_scene(ctx, NULL, <that build count>, moved_tris_with_their_mat_rows, n_tris, mats, n_mats) leaves, and the base cost becomes the
 *   new tree's.  A rebuild that fails follows the build form's rule: a HIP error or a tree higher than the stack leaves the context WITHOUT a scene.
 * - After an ordinary upload with the caller's own nodes the library has no builder to name: a limit there is RVPT_HIP_ERR_INVALID, says so, and leaves the
 *   scene untouched.  Report only (0) is legal there.
 * - On success rvpt_hip_last_error holds ONE SENTENCE (as after a PLOC build that fell back), one of
 *       guarded update: cost <%.17g>, base cost <%.17g>, limit <permille> permille: refitted
 *       guarded update: cost <%.17g>, base cost <%.17g>, limit <permille> permille: rebuilt (<lbvh|ploc|sah>), new base cost <%.17g>
 *   where `cost` is that of the refitted tree, the one the decision was taken by.  The wrappers parse this wording.
 * - Brute-force contexts hold no tree: there the guarded count is the plain update form (host arrays only), and rvpt_hip_last_error is empty afterwards.
 * - The plain update form and the three build counts behave and report exactly as before.
 * What the guard costs, and which limit separates a tree worth keeping from one worth rebuilding, is not yet measured on the device (DESIGN.md 5.10 says
 * what is open; the cost ratios of the test scenes in numpy are there).
 *
 * SPARSE UPDATE — move the listed triangles, refit only their paths:
 *
 *     rvpt_hip_upload_scene(ctx, (const rvpt_bvh_node *)indices, RVPT_HIP_NODES_UPDATE_SPARSE, tris, k, NULL, 0);      k > 0
 *
 * - With this count `nodes` is not a node array: it points at k uint32_t values, 4-byte aligned.  indices[j] is the stored triangle that tris[j] replaces, in
 *   the order the plain update form takes on this context: the leaf order after an ordinary upload, the caller's own order after a build form (the library
 *   goes through the inverse of the permutation it kept).  No index twice, none outside the stored scene.
 * - Only vert0..vert2 of each record are taken.  The stored mat_id rows, the materials, the topology and the guarded update's base cost stay.
 * - Everything is checked BEFORE anything stored is touched; a failure is RVPT_HIP_ERR_INVALID and leaves the scene as it was: no full upload on this
 *   context yet; k larger than the stored count; `nodes` NULL; materials passed; an index >= the stored count (the message names the smallest offending
 *   list position and its value); an index that occurs twice (the message names the smallest such index).  Host and device lists get the same answers.
 * - BVH contexts.  `indices` and `tris` are both host memory or both device memory of the context's GPU (16-byte aligned triangles); a mixed pair is
 *   RVPT_HIP_ERR_INVALID, so is device memory of another GPU (the message names both devices).  A device list is checked by two kernels and one read of four
 *   words.  Every touched triangle's prepared record, material index slot and unit normal are remade.  The box of every leaf that holds a touched triangle
 *   and of every node between such a leaf and the root is recomputed by the refit's rule, deepest level first, and the copies of those boxes in the
 *   4-wide form are refreshed.  EVERY OTHER BOX IS LEFT AS IT IS: a caller's loose boxes off those paths stay loose — the plain form tightens everything,
 *   this one does not.  The context then renders exactly what a full upload of (refit_bvh(nodes, patched, touched), patched, mats) renders
 *   (rvpt_amd/scene.py: refit_bvh with `touched`): images, statistics, kernel path and LDS bytes.  (The leaves of a caller's tree must not share
 *   triangles: a triangle belongs to the one leaf whose range holds it.)
 * - Brute-force contexts derive their scale, table and boxes from the whole vertex set on the host: the library reads its stored records back, patches them
 *   and runs the plain update form.  Host arrays only; a device pointer gets the plain form's answer.
 * - Frames in flight finish on the old geometry; `tris` and `indices` may be freed on return; the accumulate / reset rule stays with the caller.
 * - The plain update, the guarded update and the three build counts behave and report exactly as before.  There is no guarded sparse update.
 * Cost, 1 % of 1 M triangles on one MI355X (profiles/sparse_update.txt): from host arrays 0.32 ms for a block contiguous in the caller's
 * order and 0.52 ms scattered, against 3.53 ms for the plain update from a host array in the same run; from device memory 0.15 / 0.18 ms against 0.20 ms.
 *
 * POSE UPDATE — move parts of the mesh by one matrix each; the device poses them from a rest pose it keeps:
 *
 *     rvpt_hip_upload_scene(ctx, (const rvpt_bvh_node *)moves, RVPT_HIP_NODES_UPDATE_POSE, NULL, k, NULL, 0);      k > 0
 *
 * - With this count `nodes` is not a node array: it points at k rvpt_part_move records (64 bytes each, 4-byte aligned) in HOST memory, and `tris` is NULL.
 *   A record names the triangles [first, first + count) and carries one 3x4 matrix, row major.  `first` and `count` are in the order the plain update form
 *   takes on this context: the leaf order after an ordinary upload, the caller's own order after a build form (through the inverse of the permutation the
 *   library kept, the one the sparse update makes).  No triangle in two ranges, none outside the stored scene, no empty range; the reserved words are 0.
 * - The REST POSE is the stored vertices as they stood when the last call of any OTHER form — the full upload, a build form, the plain, guarded and sparse
 *   updates — returned successfully.  The library snapshots it at the first pose update after such a call: a device-to-device copy of the 48 vertex bytes
 *   per triangle, in stored order (a context that never poses never allocates it).  A pose update ALWAYS poses from the rest pose, never from the current
 *   position: two pose updates of one part do not compose, the second replaces the first.  A part not listed keeps the pose it has.
 *   (The SKIN UPDATE below shares this rest pose: a pose update after a skin update poses its listed parts from the rest pose and leaves the others skinned.)
 *   After any successful call of another form the next pose update takes a FRESH snapshot, and that snapshot includes whatever earlier pose updates left:
 *   pose A, a sparse update of one unrelated triangle, pose B of the same part gives B applied to the A-posed vertices.
 * - The arithmetic.  For a vertex (x, y, z) and the output component i (0, 1, 2) the value is ((m[4i]*x + m[4i+1]*y) + m[4i+2]*z) + m[4i+3]: three products
 *   and three sums, each rounded to binary32 on its own, in that order, with NO fused multiply-add.  rvpt_amd/scene.py: pose_parts is the same in numpy
 *   float32; the device, the host (brute-force contexts) and numpy agree bit for bit.  An identity matrix therefore turns a coordinate of -0.0 into +0.0
 *   (-0.0 + 0.0 is +0.0): that is what the arithmetic gives.  Non-finite matrix entries are the caller's problem, as non-finite vertices are.
 * - Only the vertices move: the x, y, z of vert0..vert2.  Their w lanes come from the rest pose; the stored mat_id rows, the materials, the topology, the
 *   permutation and the guarded update's base cost stay.
 * - Everything is checked BEFORE anything stored is touched; a failure is RVPT_HIP_ERR_INVALID, has a message, and leaves the scene and the rest pose as they
 *   were: no full upload on this context yet; k == 0; k larger than the stored count; `moves` NULL; `moves` not 4-byte aligned; `tris` not NULL; materials
 *   passed; `moves` in device memory (this form takes its list from the host); then, record by record in list order, a count of 0, a non-zero reserved
 *   word, first + count past the stored count (computed without overflow) — the message names the smallest offending list position; then two ranges that share
 *   a triangle — the message names the smallest pair of list positions (i, j), i < j, whose ranges meet.
 * - BVH contexts.  Every listed triangle's vertex rows are written, its prepared record, material index slot and unit normal are remade; the box of every leaf
 *   that holds a listed triangle and of every node from there to the root is recomputed by the refit's rule, deepest level first; the wide form's copies are
 *   refreshed; EVERY OTHER BOX IS LEFT AS IT IS, as in the sparse update.  The context then renders exactly what a full upload of
 *   (refit_bvh(nodes, posed, touched = the listed positions), posed, mats) renders: images, statistics and kernel path.  (The 4-wide form keeps the grouping
 *   the upload made, as after every update form; a fresh upload of a tree moved far may group its children anew and then asks for other LDS bytes, never for
 *   another image.)  Ray and path queries answer on the posed scene with `prim` numbered as before.
 * - Brute-force contexts keep the rest pose on the host: the stored records are read back, the listed ranges are posed there, and the plain update form runs,
 *   as the sparse form does there.
 * - Frames in flight finish on the old geometry; `moves` may be freed on return; the accumulate / reset rule stays with the caller; rvpt_hip_last_error is
 *   empty afterwards.  The GUARDED POSE UPDATE below is this form with the tree costed behind it and rebuilt past a limit.  The laboratory's caller-layout
 *   knob has no sparse form and so no pose form: the same error.
 * - Every other form behaves and reports exactly as before.
 * Cost on one MI355X: profiles/pose_update.txt; DESIGN.md 5.16.
 *
 * GUARDED POSE UPDATE — the pose update, then the cost of the posed tree, and a rebuild once it has gone stale; the rest pose survives the rebuild:
 *
 *     rvpt_hip_upload_scene(ctx, (const rvpt_bvh_node *)moves, RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille), NULL, k, NULL, 0);      k > 0
 *
 * permille is 0 (report only) or 1000 .. 65535, the guarded update's limit.  Any other value in the band is RVPT_HIP_ERR_INVALID and leaves the stored scene
 * and the rest pose untouched.
 * - BVH contexts.  Every refusal of the pose update comes first, in its words and its order.  Then the one refusal of this form: a limit on a tree that came
 *   from an ordinary upload with the caller's own nodes is RVPT_HIP_ERR_INVALID — the library has no builder to name —, decided before anything is touched.
 *   Report only (0) is legal there.
 * - The pose update runs exactly as above: the snapshot if the context holds no rest pose, the listed rows posed from it, the boxes on their paths refitted.
 *   Then the TREE COST of the stored tree is computed as in the guarded update; the boxes off the listed paths enter it as they are, loose ones included.
 *   The base cost is the guarded update's.
 * - With a limit, if cost > (permille / 1000) * base cost and the stored scene came from a build form, the library REBUILDS with that build form's method from
 *   the posed vertices beside the stored mat_id rows, carried back into the caller's order, and the materials as the caller last passed them.  What the
 *   context then holds — tree, permutation, level table, wide form, launch choice — is what
 *   rvpt_hip_upload_scene(ctx, NULL, <that build count>, posed_in_caller_order, n_tris, mats, n_mats) leaves, and the base cost becomes the new tree's.
 * - THE REST POSE GOES WITH THE REBUILD.  Its 48 bytes per triangle are carried into the caller's order by the old permutation and gathered back by the new
 *   one, on the device (a second buffer of 48 bytes per triangle, allocated at the first such rebuild of a context).  The next pose update — plain or
 *   guarded — poses from the same rest pose as before the rebuild: a caller sends absolute poses frame after frame, and they never compose.  A part not
 *   listed keeps the pose it has.  `first` and `count` stay in the caller's order, as after any build form.
 * - A successful call of this form, like one of the plain pose form, keeps the rest pose.  A rebuild that fails follows the build form's rule: the context is
 *   left WITHOUT a scene, and the rest pose is dropped with it.
 * - On success rvpt_hip_last_error holds ONE SENTENCE, one of
 *       guarded pose update: cost <%.17g>, base cost <%.17g>, limit <permille> permille: refitted
 *       guarded pose update: cost <%.17g>, base cost <%.17g>, limit <permille> permille: rebuilt (<lbvh|ploc|sah>), new base cost <%.17g>
 *   where `cost` is that of the posed tree, the one the decision was taken by, and the name is that of the tree the scene then holds (a PLOC rebuild that
 *   fell back names lbvh; the next rebuild is a PLOC build again).  The wrappers parse this wording.
 * - Brute-force contexts hold no tree: there the count is the plain pose update, and rvpt_hip_last_error is empty afterwards.
 * - Frames in flight finish on the old geometry; `moves` may be freed on return.  Every other form, the plain pose update included, behaves and reports
 *   exactly as before, and after each of the others the next pose update takes a fresh snapshot.
 * Measured on one MI355X, 1 M triangles (profiles/guarded_pose.txt): the guard adds 0.045 ms to the 0.140 ms pose of a 1 % part; a call that
 * rebuilds takes 2.2 / 3.5 / 15.1 ms (LBVH / PLOC / SAH); a tenth of the mesh rotated by 2 degrees reports a ratio of 1.33 with the tree at 0.40 of a rebuilt
 * one's rate, the same part carried across the scene 226.  A limit at or below 1.3 catches the first; nothing finer was measured.
 *
 * BIND — four bone indices and four weights per vertex, kept by the library for the skin update below:
 *
 *     rvpt_hip_upload_scene(ctx, (const rvpt_bvh_node *)skin, RVPT_HIP_NODES_BIND_SKIN, NULL, n_tris, NULL, 0);
 *
 * - `skin` points at 3 * n_tris rvpt_vertex_skin records (32 bytes each); record 3 t + v belongs to vertex v of triangle t, and t is numbered in the order the
 *   plain update form takes on this context: the leaf order after an ordinary upload, the caller's own order after a build form.  The library keeps its copy
 *   IN THAT ORDER (96 bytes per triangle, one device buffer, freed with the context) and goes through the stored permutation when it skins: a guarded rebuild,
 *   which changes the permutation and not the update order, leaves the binding valid.
 * - `skin` may be host memory (4-byte aligned); on BVH contexts also device memory of the context's GPU, 16-byte aligned.  Brute-force contexts keep the
 *   binding on the host and take host memory only.
 * - Refusals, RVPT_HIP_ERR_INVALID with a message, decided in this order before anything is touched — the earlier binding stays: no scene; n_tris is not the
 *   stored count; `skin` NULL; `skin` misaligned; `tris` not NULL; materials passed; device memory of another GPU (both devices named) or a device pointer on a
 *   brute-force context; a bone[j] >= RVPT_HIP_SKIN_MAX_BONES — the message names the smallest offending record position, its j and the value, the same for
 *   host and device lists (a device list is checked by one kernel and one read of four words).
 * - The bind records the LARGEST BONE INDEX of the list and the smallest record position that holds it: a skin update needs more matrices than that.
 * - It moves nothing.  It is not "another form" in the pose update's snapshot rule: the rest pose stays.  The slots' prepared state stays, rvpt_hip_last_error
 *   is empty afterwards, and a frame after a bind is bit for bit the frame without it.  A second bind replaces the first.
 * - The binding is DROPPED by an ordinary full upload, by a build form the caller asks for, and whenever a call leaves the context without a scene.  It
 *   SURVIVES the plain, guarded, sparse, pose and guarded pose updates, their rebuilds included.  It survives the guarded skin update and its rebuild too.
 * - Weights are taken as given: they need not sum to 1, and non-finite weights are the caller's problem.
 *
 * SKIN UPDATE — linear blend skinning: every vertex of the mesh posed from the rest pose by its four weighted bone matrices, on the device:
 *
 *     rvpt_hip_upload_scene(ctx, (const rvpt_bvh_node *)bones, RVPT_HIP_NODES_UPDATE_SKIN, NULL, k, NULL, 0);      0 < k <= RVPT_HIP_SKIN_MAX_BONES
 *
 * - `bones` points at k rvpt_bone records (48 bytes: a 3x4 matrix, row major, as rvpt_part_move::m) in host memory (4-byte aligned) or, on BVH contexts, in
 *   device memory of the context's GPU, 16-byte aligned (a tensor an animation system wrote; the caller guarantees that the writer has finished).
 * - The arithmetic.  For a vertex with rest position p and influences j = 0..3: q_j = pose(M[bone[j]], p), where pose is EXACTLY the pose update's arithmetic
 *   (((m0 x + m1 y) + m2 z) + m3 per component), and out_i = ((w0*q0_i + w1*q1_i) + w2*q2_i) + w3*q3_i: four products and three sums, each rounded to
 *   binary32 on its own, in that order, with NO fused multiply-add anywhere.  All four influences are always evaluated: a zero weight contributes 0 * q.
 *   One-hot weights therefore reproduce the pose update's bytes, up to -0 + 0 = +0.  rvpt_amd/scene.py: skin_triangles is the same in numpy float32; the
 *   device, the host (brute-force contexts) and numpy agree bit for bit.  The w lanes come from the rest pose; the stored mat_id rows, the materials, the
 *   topology, the permutation and the guarded update's base cost stay.  Non-finite matrix entries are the caller's problem.
 * - THE REST POSE IS THE POSE UPDATE'S: the same buffer, the same flag, the same rule.  It is snapshotted by the first pose OR skin update after a successful
 *   call of any form that is not a pose update, a guarded pose update, a skin update or a bind.  A skin update always skins from it, writes EVERY triangle, and
 *   keeps it: two skin updates never compose.
 * - Every box is then refitted by the PLAIN form's rule (every level, deepest first, then the wide copies), and prepared records, material slots and unit
 *   normals are remade.  The context then renders exactly what the plain update form, called with the skinned vertices, renders — images, statistics, kernel
 *   path —, which is a fresh upload of (refit_bvh(nodes, skinned), skinned, mats) with the wide grouping kept as after every update form.  Loose boxes become
 *   tight, as after a plain update.  Ray and path queries answer on the skinned scene, with `prim` numbered as before.
 * - Brute-force contexts work on the host: the stored records are read back, the rest pose is kept on the host, the vertices are skinned there with the same
 *   unfused arithmetic, and the plain update form runs.
 * - Refusals, in this order, decided before anything stored is touched — the scene, the rest pose and the binding are left as they were: no scene; k == 0;
 *   k > RVPT_HIP_SKIN_MAX_BONES; `bones` NULL; `bones` misaligned; `tris` not NULL; materials passed; no binding ("skin update before a bind"); k <= the
 *   largest bound bone index (the message names the index, the record position that holds it, and k); device memory of another GPU; a device pointer on a
 *   brute-force context; the laboratory's caller-layout knob, with the answer the plain form gives.
 * - Frames in flight finish on the old geometry; `bones` may be freed on return; rvpt_hip_last_error is empty afterwards.  Every other form behaves and reports
 *   exactly as before.  There is NO GUARDED SKIN UPDATE: the tree is refitted, never costed or rebuilt, by this form; a caller whose skinned mesh has left its
 *   tree behind runs a guarded update or a build form.  (That is this count's rule.  The GUARDED SKIN UPDATE below is this form under a count of its own, with
 *   the tree costed behind it and rebuilt past a limit, and it keeps the binding and the rest pose.)
 * Cost on one MI355X: profiles/skin_update.txt; DESIGN.md 5.18.
 *
 * GUARDED SKIN UPDATE — the skin update, then the cost of the skinned tree, and a rebuild once it has gone stale; the rest pose and the binding survive the rebuild:
 *
 *     rvpt_hip_upload_scene(ctx, (const rvpt_bvh_node *)bones, RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille), NULL, k, NULL, 0);      0 < k <= RVPT_HIP_SKIN_MAX_BONES
 *
 * permille is 0 (report only) or 1000 .. 65535, the guarded update's limit.  Any other value in the band is RVPT_HIP_ERR_INVALID ("guarded skin update: the
 * limit is 0 (report only) or 1000 .. 65535 permille, got <n>") and leaves the stored scene, the rest pose and the binding untouched.  `bones` is the skin
 * update's list: host memory or, on BVH contexts, device memory of the context's GPU.
 * - BVH contexts.  Every refusal of the skin update comes first, in its words and its order.  Then the one refusal of this form: a limit on a tree that came
 *   from an ordinary upload with the caller's own nodes is RVPT_HIP_ERR_INVALID — the library has no builder to name —, decided before anything is touched.
 *   Report only (0) is legal there.
 * - The skin update runs exactly as above: the snapshot if the context holds no rest pose, every vertex skinned from it, every box refitted by the plain
 *   form's rule.  Then the TREE COST of the stored tree is computed as in the guarded update; every box is tight.  The base cost is the guarded update's.
 * - With a limit, if cost > (permille / 1000) * base cost (in double) and the stored scene came from a build form, the library REBUILDS with that build form's
 *   method from the skinned vertices beside the stored mat_id rows, carried back into the caller's order, and the materials as the caller last passed them.
 *   What the context then holds — tree, permutation, level table, wide form, launch choice — is what
 *   rvpt_hip_upload_scene(ctx, NULL, <that build count>, skinned_in_caller_order, n_tris, mats, n_mats) leaves, and the base cost becomes the new tree's.
 * - THE REST POSE GOES WITH THE REBUILD, as in the guarded pose update: into the caller's order by the old permutation, back into stored order by the new one.
 *   THE BINDING STAYS WHERE IT IS: it is kept in the caller's order and read through the stored permutation, so the new permutation is all it needs.  The
 *   largest bound bone index and its position stay.  The next skin update — plain or guarded — poses every vertex from the same rest pose through the same
 *   weights as before the rebuild, and the next pose update poses from that rest pose too.
 * - A successful call of this form, like one of the plain skin form, keeps the rest pose and the binding, and the context remembers k matrices.  A rebuild that
 *   fails follows the build form's rule: the context is left WITHOUT a scene, and the rest pose and the binding are dropped with it.
 * - On success rvpt_hip_last_error holds ONE SENTENCE, one of
 *       guarded skin update: cost <%.17g>, base cost <%.17g>, limit <permille> permille: refitted
 *       guarded skin update: cost <%.17g>, base cost <%.17g>, limit <permille> permille: rebuilt (<lbvh|ploc|sah>), new base cost <%.17g>
 *   where `cost` is that of the skinned tree, the one the decision was taken by, and the name is that of the tree the scene then holds (a PLOC rebuild that
 *   fell back names lbvh; the next rebuild is a PLOC build again).  The wrappers parse this wording.
 * - Brute-force contexts hold no tree: there the count is the plain skin update, and rvpt_hip_last_error is empty afterwards.
 * - Frames in flight finish on the old geometry; `bones` may be freed on return.  Every other form, the plain skin update included, behaves and reports
 *   exactly as before.
 * Measured on one MI355X, 1 M triangles, 64 bones (profiles/guarded_skin.txt): the guard adds 0.045 ms to the 0.207 ms skin update; a call that
 * rebuilds takes 2.2 / 3.5 / 17.0 ms (LBVH / PLOC / SAH); a fold of the bone grid by a tenth of the extent reports a ratio of 1.09, by a half 1.32.  The rate on
 * the folded trees was not measured: no limit is recommended for a skinned mesh. */
typedef struct rvpt_vertex_skin {    /* 32 bytes: the four influences of ONE vertex */
    uint32_t bone[4];                /* indices into the skin update's matrices, each < RVPT_HIP_SKIN_MAX_BONES */
    float    weight[4];
} rvpt_vertex_skin;
typedef struct rvpt_bone {           /* 48 bytes */
    float    m[12];                  /* 3x4, row major, as rvpt_part_move::m */
} rvpt_bone;
#define RVPT_HIP_SKIN_MAX_BONES 1024u
#define RVPT_HIP_NODES_BIND_SKIN ((size_t)-6)
#define RVPT_HIP_NODES_UPDATE_SKIN ((size_t)-7)
#define RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille) ((size_t)0 - (size_t)(0x300000u + (permille)))
typedef struct rvpt_part_move {      /* 64 bytes */
    float    m[12];                  /* 3x4, row major: x' = m[0] x + m[1] y + m[2] z + m[3], y' from m[4..7], z' from m[8..11] */
    uint32_t first, count;           /* the triangles [first, first + count) */
    uint32_t reserved[2];            /* must be 0 */
} rvpt_part_move;
#define RVPT_HIP_NODES_UPDATE_POSE ((size_t)-5)
#define RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) ((size_t)0 - (size_t)(0x200000u + (permille)))
#define RVPT_HIP_NODES_UPDATE_GUARDED(permille) ((size_t)0 - (size_t)(0x10000u + (permille)))
#define RVPT_HIP_NODES_BUILD ((size_t)-1)
#define RVPT_HIP_NODES_BUILD_PLOC ((size_t)-2)
#define RVPT_HIP_NODES_BUILD_SAH ((size_t)-3)
#define RVPT_HIP_NODES_UPDATE_SPARSE ((size_t)-4)
int rvpt_hip_upload_scene(rvpt_hip_ctx *ctx, const rvpt_bvh_node *nodes, size_t n_nodes,
                          const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats,
                          size_t n_mats);

/* Replaces the settings + camera uniform copies (rvpt.cpp:118,120).  The accumulate/reset
 * rule (rvpt.cpp:21-29,102-111) stays with the caller: settings->current_frame is
 * authoritative, 0 means "ignore the accumulator". */
int rvpt_hip_set_frame(rvpt_hip_ctx *ctx, const rvpt_render_settings *settings,
                       const rvpt_camera_data *camera);

/* Replaces record_compute_command_buffer() + queue submit (rvpt.cpp:1005-1039,352-354):
 * asynchronous enqueue of one frame.  Up to `frames_in_flight` frame kernels overlap on the device (they
 * write per-frame sample buffers); the temporal blend into the accumulator runs in dispatch order. */
int rvpt_hip_dispatch(rvpt_hip_ctx *ctx);

/* The reference's steady state — camera and settings unchanged, update() only increments current_frame
 * (rvpt.cpp:102-111) — as one call: enqueues the n_frames consecutive frames settings->current_frame ...
 * current_frame + n_frames - 1 of the last set_frame().  The accumulator ends up bit-identical to n_frames calls of
 * set_frame(current_frame + k) / dispatch(); the frames share one kernel launch (work items = frames x pixels, one
 * temporal-blend pass applying the frames in order), which removes the per-frame ramp-up and drain from the
 * device time.  The caller advances its frame counter by n_frames.  1 <= n_frames <= RVPT_HIP_MAX_FRAMES_PER_DISPATCH. */
#define RVPT_HIP_MAX_FRAMES_PER_DISPATCH 64u
int rvpt_hip_dispatch_frames(rvpt_hip_ctx *ctx, uint32_t n_frames);

/* Replaces raytrace_work_fence.wait()/reset() (rvpt.cpp:115-116).  query: 0 done, 1 pending. */
int rvpt_hip_wait(rvpt_hip_ctx *ctx);
int rvpt_hip_query(rvpt_hip_ctx *ctx);
/* Fence::wait with its timeout (vk_util.cpp:65,94-97: DEFAULT_FENCE_TIMEOUT = 1 s, result ignored upstream): waits at
 * most timeout_ns for everything dispatched so far.  0 done, 1 still pending when the time was up, negative error. */
int rvpt_hip_wait_for(rvpt_hip_ctx *ctx, uint64_t timeout_ns);

/* Host read-back of the frame (the reference only samples output_image in its blit,
 * rvpt.cpp:851-852,960-964).  Row-major, top row first, width*height*4 components.  Implies rvpt_hip_wait.
 * Partitioned image (tile_world > 1):
 *   - with a communicator (rvpt_hip_comm_init / rvpt_hip_comm_init_all) the call is COLLECTIVE: every rank calls it, the
 *     per-tile radiance is gathered to rank 0 over RCCL and un-tiled there; rank 0 receives the whole frame, the other ranks
 *     only send (their dst may be NULL and is not written).  In a single-process group only rank 0's context is called;
 *   - without one, pixels of tiles this rank does not own read as 0 (a host doing its own exchange uses
 *     rvpt_hip_tile_buffer / rvpt_hip_untile).
 * FRAMES THAT STAY ON THE DEVICE: `dst` may be device memory of the context's GPU (hipMalloc: a torch tensor's storage, say; pinned and managed memory
 * count as host memory, as for the triangles of rvpt_hip_upload_scene).  Both formats; the bytes written are exactly the bytes a host read of the same
 * state returns.  Without a communicator the un-tiling kernel writes straight into `dst` (RGBA8: un-tiled and quantised in one kernel) — no staging
 * buffer, no second copy; with one, rank 0 gathers as for a host read and the frame (RGBA8: quantised) goes from the staging buffer into `dst` on the
 * device, and the rule that rank 0 takes part in the exchange before it reports its own bad argument stays.  `dst` need only be 4-byte aligned.  The
 * call still implies rvpt_hip_wait and returns only after the context's stream has finished writing `dst`: the caller may then read it from any stream
 * of its own.  dst_bytes too small is RVPT_HIP_ERR_SIZE, device memory of another GPU RVPT_HIP_ERR_INVALID (the message names both devices), so is
 * device memory that is not 4-byte aligned; in every such case `dst` is untouched.
 *
 * RAY QUERIES — closest and any hit for the caller's own rays, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_RAY_HITS, records, n * sizeof(rvpt_ray_hit));
 *
 * `dst` then holds n rvpt_ray_hit records: each comes in as a ray (org, tmax, dir, flags) and goes out as a hit (t, prim, u, v).  The in fields are never written.
 * - THE ORDER A QUERY WALKS.  BVH contexts (RVPT_HIP_TRAVERSAL_BVH and RVPT_HIP_TRAVERSAL_BVH_ORDERED alike): intersect_bvh of the reference
 *   (intersection.glsl:361-413) — left child first, closest-t starts at tmax, a triangle is accepted iff 0 < t < closest, 0 < u, 0 < v and u + v < 1.  Brute-force
 *   contexts: triangles 0 .. n-1 in stored order with the same shrinking interval.  A query never uses the nearer-child-first order: its answer is defined by one
 *   order per kind of context, not by a create flag.  `dir` need not be normalised, t is in units of `dir`; zero components of `dir` get what the arithmetic
 *   gives (1.0f / 0), as they do in a frame.
 * - WHAT A RECORD HOLDS ON RETURN.  Closest hit: t is the accepted distance, u and v the two values the accepting test computed, prim the triangle.  With
 *   RVPT_HIP_RAY_ANY_HIT: the same fields for the FIRST triangle accepted in that order; the walk stops there.  Miss: prim = 0xFFFFFFFF, t = the bits of tmax as
 *   given, u = v = 0.  A ray with a non-finite component in org or dir is a miss, decided before the walk; so is a tmax that is NaN, zero or negative.
 * - THE NUMBERING OF prim follows the order the plain update form takes on this context: the stored order (the leaf order the caller uploaded) after an
 *   ordinary upload, the CALLER'S order after a build form (through the stored permutation).
 * - The call needs a scene — before any full upload it is RVPT_HIP_ERR_INVALID; the empty scene answers every ray with a miss — and no rvpt_hip_set_frame.
 *   dst_bytes must be a multiple of 48, else RVPT_HIP_ERR_INVALID; dst_bytes == 0 is a successful no-op; fewer than 2^32 records per call.
 * - `dst` is host memory or device memory of the context's GPU, classified as for frames.  Device memory must be 16-byte aligned, else RVPT_HIP_ERR_INVALID;
 *   another GPU's memory is RVPT_HIP_ERR_INVALID naming both devices.  In every error case `dst` is untouched.  Host records go through a staging buffer the
 *   context grows; device records never visit the host, and the call returns after the context's stream has finished writing them.
 * - The call is LOCAL: with a communicator it is not collective and touches no peer.  Every rank holds the whole scene, and any rank answers.
 * - It implies rvpt_hip_wait, as every read does, and leaves untouched the accumulator, rvpt_hip_get_timing, rvpt_hip_get_stats, rvpt_hip_get_launch_info,
 *   rvpt_hip_get_cull_info, the frame counter, and rvpt_hip_last_error on success: a frame dispatched after a query is bit for bit the frame dispatched without it.
 * DESIGN.md 5.13 has the kernels and what was measured (profiles/ray_queries.txt).
 *
 * K-NEAREST RAY QUERIES — the first k hits along the caller's own rays, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k), records, n * k * sizeof(rvpt_ray_hit));      k = 1 .. RVPT_HIP_RAY_MAX_HITS
 *
 * `dst` then holds n GROUPS of k consecutive rvpt_ray_hit records.  Record 0 of a group carries the ray in its in fields (org, tmax, dir, flags); the in fields
 * of records 1 .. k-1 are ignored.  No in field of any record is ever written.  On return the out quad (t, prim, u, v) of record j holds the j-th hit of the
 * group's ray.  The k belongs to the call, not to the record: a launch is uniform in k.  Formats 32 and 41 are the "unknown format" error.
 * - THE ANSWER IS DEFINED BY THE WALK, as a ray query's is: the order is THE ORDER A QUERY WALKS above — intersect_bvh of the reference, left child first, on
 *   BVH contexts under both BVH traversal flags; triangles 0 .. n-1 in stored order on brute-force contexts.  A valid ray keeps a list H of at most k accepted
 *   hits and a value `bound` that starts at tmax.
 * - CLOSEST MODE (flags without RVPT_HIP_RAY_ANY_HIT).  Every box test and every triangle test uses the interval (0, bound).  A triangle is accepted iff
 *   0 < t < bound, 0 < u, 0 < v and u + v < 1: the tests of a ray query.  An accepted hit is inserted behind every entry whose t is <= its own: among equal t
 *   the one accepted earlier stays in front.  If H then holds k + 1 entries, the last is dropped.  Whenever H holds k entries, `bound` is the t of the last.
 *   A later triangle at exactly the k-th t is therefore not accepted: the test is strict, as a ray query's is.
 * - ANY-HIT MODE (the bit set in record 0).  `bound` stays tmax, accepted hits are appended in the order of acceptance, and the walk stops when H holds k:
 *   record j is the j-th triangle accepted.
 * - WHAT A GROUP HOLDS ON RETURN.  For j < |H| the quad of record j is (t, prim, u, v) of the j-th entry: u and v are what the accepting test computed, prim is
 *   numbered as a ray query numbers it (THE NUMBERING OF prim above).  For j >= |H| it is the miss quad of a ray query: t = the bits of record 0's tmax as
 *   given, prim = 0xFFFFFFFF, u = v = 0.  A ray with a non-finite component in org or dir, or a tmax that is NaN, zero or negative, gets k miss quads, decided
 *   before the walk.
 * - With k = 1 both modes are format 2 exactly: RVPT_HIP_FORMAT_RAY_HITS_NEAREST(1) is format 2, the same kernels and the same bytes.
 * - ON BRUTE-FORCE CONTEXTS the closest-mode answer is therefore the first k of all triangles accepted in (0, tmax), ordered by (t, stored index).  On BVH
 *   contexts the visiting order decides among equal t, as it does for a ray query.
 * - Everything else is a ray query's rule: the call needs a scene and no rvpt_hip_set_frame, the empty scene answers with misses; dst_bytes must be a multiple
 *   of 48 * k, else RVPT_HIP_ERR_INVALID (the message gives k and the byte count); dst_bytes == 0 is a successful no-op; fewer than 2^32 records (n * k) per
 *   call; `dst` is host memory or 16-byte aligned device memory of the context's GPU, another GPU's memory is an error naming both devices, and in every error
 *   case `dst` is untouched; the call is LOCAL under a communicator, implies rvpt_hip_wait, and leaves untouched what a ray query leaves untouched.
 * DESIGN.md 5.23 has the kernels and what was measured (profiles/ray_queries.txt).
 *
 * RAY CROSSINGS — how many surfaces the caller's own rays pass, by facing, and over what stretch, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_RAY_CROSSINGS, records, n * sizeof(rvpt_ray_crossings));
 *
 * `dst` then holds n rvpt_ray_crossings records: each comes in as a ray (org, tmax, dir; flags is reserved and ignored, RVPT_HIP_RAY_ANY_HIT included) and goes
 * out as (front, back, t_near, t_far).  The in fields are never written.
 * - A VALID RAY is a ray query's: a non-finite component of org or dir, or a tmax that is NaN, zero or negative, is decided before any walk, and such a ray
 *   is answered as a ray with no crossing.
 * - THE SET A is every triangle test accepted by the walk of an any-hit k-nearest ray query with no limit on k.  The order is THE ORDER A QUERY WALKS above.
 *   `bound` stays tmax from start to end: every box test and every triangle test uses the interval (0, tmax), and a triangle is accepted iff 0 < t < tmax,
 *   0 < u, 0 < v and u + v < 1.  On brute-force contexts every stored triangle is tested; on BVH contexts the tested triangles are those under the leaves the
 *   reference's walk reaches with that fixed interval.
 * - A DOES NOT DEPEND ON THE VISITING ORDER, because the interval never changes: the answer is the same under RVPT_HIP_TRAVERSAL_BVH,
 *   RVPT_HIP_TRAVERSAL_BVH_ORDERED and RVPT_HIP_BVH_PER_LANE.  Stacked duplicates count once each.  Each stored triangle is taken to lie under one leaf; a
 *   caller's tree that lists a triangle under two leaves counts it twice.
 * - FACING.  n is the stored unit normal of the accepted triangle, the 12 bytes SURFACE POINTS returns.  s = (dir.x*n.x + dir.y*n.y) + dir.z*n.z in binary32,
 *   every operation rounded on its own, no FMA.  The hit is FRONT iff s < 0; every other hit is BACK (s > 0, s == 0, s NaN), hence front + back == |A|.  For a
 *   closed mesh with outward normals, back - front is 1 from inside and 0 from outside along any ray that meets no edge exactly.
 * - WHAT A RECORD HOLDS ON RETURN.  front and back are the two counts; t_near and t_far are the smallest and the largest accepted t (accepted t are finite, so
 *   min and max are order-free).  If A is empty: front = back = 0, t_near = the bits of tmax as given (a NaN's payload included), t_far = +0.0.
 * - WHAT IS NOT PROMISED.  On brute-force contexts t_near equals format 2's t.  On BVH contexts the closest-hit walk tests boxes against a shrinking interval,
 *   and equality is not promised there; nor is it promised that a BVH context's A equals the brute-force context's A over the same triangles: a box test
 *   may turn away a ray that its triangle's test would accept.
 * - COST.  A crossing ray tests every triangle whose leaf its line enters inside (0, tmax): at most n_tris per ray, which a brute-force ray query already
 *   costs.  A finite tmax is the caller's bound.
 * - Everything else is a ray query's rule: the call needs a scene and no rvpt_hip_set_frame, the empty scene answers with no crossing; dst_bytes must be a
 *   multiple of 48, else RVPT_HIP_ERR_INVALID; dst_bytes == 0 is a successful no-op; fewer than 2^32 records per call; `dst` is host memory or 16-byte aligned
 *   device memory of the context's GPU, another GPU's memory is an error naming both devices, and in every error case `dst` is untouched; for host records
 *   only the out quad travels back; the call is LOCAL under a communicator, implies rvpt_hip_wait, leaves untouched what a ray query leaves untouched, and
 *   answers on the scene as the last update form left it.
 * DESIGN.md 5.27 has the kernels and what was measured (profiles/ray_crossings.txt).
 *
 * PATH QUERIES — radiance along the caller's own rays, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_RAY_PATHS, records, n * sizeof(rvpt_ray_path));
 *
 * `dst` then holds n rvpt_ray_path records: each comes in as a ray, an RNG state and a bounce budget (org, seed, dir, max_bounces) and goes out as a radiance and
 * a count (radiance, segments).  The in fields are never written.
 * - WHAT A RECORD HOLDS ON RETURN.  radiance is what integrator_Kajiya (integrators.glsl:571-671) returns for the ray (org, dir): the function a frame's mode-9
 *   pixel evaluates after its camera ray is made, run with the record's max_bounces and with the RNG state `seed` — every rand() of the path advances that state
 *   as util.glsl:38-50 does.  segments is the number of closest-hit queries the path made: what RVPT_HIP_COUNT_SEGMENTS counts, per path.  radiance is the
 *   integrator's value itself: a frame adds it to zero, which turns -0 into +0; the query does not.
 * - THE ORDER A PATH WALKS is a ray query's, for every segment: intersect_bvh of the reference on BVH contexts (RVPT_HIP_TRAVERSAL_BVH_ORDERED contexts too),
 *   stored order on brute-force contexts, each segment with the interval (0, +inf).  A path query's bits therefore depend on no create flag other than brute
 *   force against BVH.
 * - INVALID RECORDS.  A record is invalid if a component of org or dir is non-finite, if max_bounces == 0 or if max_bounces > RVPT_HIP_PATH_MAX_BOUNCES.  That is
 *   decided before any walk and answered radiance = 0, 0, 0 and segments = 0 — as the reference's loop integrators return black without tracing for a
 *   non-positive budget (integrators.glsl:574).  The upper bound is not a convenience: a mirror box with a budget of 2^32 would hold a shared GPU for minutes,
 *   and no input may make a launch unbounded.
 * - A seed of 0 is legal: xorshift32 then stays 0, which is what the arithmetic gives.
 * - The call needs a scene — before any full upload it is RVPT_HIP_ERR_INVALID; the empty scene answers every valid record with the miss radiance of its dir and
 *   segments = 1 — and no rvpt_hip_set_frame.  dst_bytes must be a multiple of 48, else RVPT_HIP_ERR_INVALID; dst_bytes == 0 is a successful no-op; fewer than
 *   2^32 records per call.
 * - `dst` is host memory or device memory of the context's GPU, classified as for frames.  Device memory must be 16-byte aligned, else RVPT_HIP_ERR_INVALID;
 *   another GPU's memory is RVPT_HIP_ERR_INVALID naming both devices.  In every error case `dst` is untouched.  Host records go through the ray queries' staging
 *   buffer, and only the out fields travel back; device records never visit the host.
 * - The call is LOCAL: with a communicator it is not collective and touches no peer.
 * - It implies rvpt_hip_wait and leaves untouched the accumulator, rvpt_hip_get_timing, rvpt_hip_get_stats, rvpt_hip_get_launch_info, rvpt_hip_get_cull_info,
 *   the frame counter, and rvpt_hip_last_error on success: a frame dispatched after a path query is bit for bit the frame dispatched without it.
 * - THE OTHER INTEGRATORS, PER CALL.  rvpt_hip_read(ctx, RVPT_HIP_FORMAT_RAY_PATHS_MODE(m), records, n * sizeof(rvpt_ray_path)), m = 0 .. 9, is this form with
 *   every record evaluated by the integrator of render mode m (compute_pass.comp:76-95: 0 binary, 1 color, 2 depth, 3 normal, 4 Utah, 5 ambient occlusion,
 *   6 Appel, 7 Whitted, 8 Cook, 9 Kajiya) instead of integrator_Kajiya.  The mode belongs to the call, not to the record: a launch is uniform in its integrator.
 *   Mode 9 (format 25) IS format 3: the same kernels and the same bytes.  max_bounces is what the integrator receives as render_settings.max_bounces: the bounce
 *   budget of Whitted, Cook and Kajiya, the number of occlusion samples of integrator_ao; modes 0-4 and 6 ignore it.  The validity rule above holds for EVERY
 *   mode, those that ignore the budget included; a frame with max_bounces <= 0 is therefore not reproduced for the modes that would still trace (0-6: such a
 *   frame's ambient occlusion is 1 - 0/0) — one rule for all modes is worth more than that corner.  segments counts every closest-hit query the record made,
 *   shadow and occlusion queries included: what RVPT_HIP_COUNT_SEGMENTS counts in a frame of that mode.  Everything else is as written above for format 3.
 * - HART IS NOT PART OF THIS FORM: mode 10 and every mode eval_integrator sends to its default branch.  integrator_Hart marches 32 steps over all triangles per
 *   ray, and on a large scene no record count keeps such a launch bounded — the rule RVPT_HIP_PATH_MAX_BOUNCES exists for.  Format 26 and every other value are
 *   the "unknown format" error.
 * DESIGN.md 5.14 has the kernels and what was measured (profiles/path_queries.txt); 5.21 has the integrators per call (profiles/path_modes.txt).
 *
 * NEAREST POINTS — the nearest point of the mesh to the caller's own points, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_NEAREST_POINTS, records, n * sizeof(rvpt_point_hit));
 *
 * `dst` then holds n rvpt_point_hit records: each comes in as a point and a bound (point, max_d2) and goes out as the nearest point of the mesh (closest, d2,
 * prim, u, v, region).  The in fields are never written.  max_d2 and d2 are SQUARED distances: there is no square root in this form.
 * - THE ANSWER IS DEFINED WITHOUT REFERENCE TO ANY WALK.  Every stored triangle i gets a candidate (d2_i, prim_i) by the arithmetic below; the answer is the
 *   lexicographically smallest candidate that is smaller than (max_d2, 0xFFFFFFFF).  A candidate whose d2 is NaN never wins (< and == are both false for it).
 *   So d2 == max_d2 is accepted, max_d2 == 0 finds a point on the surface, and among equal d2 the smaller reported prim wins.  (On a BVH context the stored
 *   triangles are those under the leaves of the tree, as for a ray.)
 * - THE NUMBERING OF prim is a ray query's: the stored order after an ordinary upload, the CALLER'S order after a build form (through the stored
 *   permutation).  The tie is broken on that reported number, so the answer does not depend on which builder made the tree.
 * - PER-TRIANGLE ARITHMETIC.  binary32 throughout; every product, sum and quotient is rounded on its own, no FMA.  a, b, c = vert0..2 of the stored row, p = point.
 *     ab = b-a, ac = c-a, ap = p-a, bp = p-b, cp = p-c;   dot(x,y) = (x0*y0 + x1*y1) + x2*y2;
 *     d1 = dot(ab,ap), d2' = dot(ac,ap), d3 = dot(ab,bp), d4 = dot(ac,bp), d5 = dot(ab,cp), d6 = dot(ac,cp);
 *     vc = d1*d4 - d3*d2', vb = d5*d2' - d1*d6, va = d3*d6 - d5*d4.
 *   The regions (the Voronoi regions of Ericson's point-triangle test) are tested in this order, and the first that holds decides (u, v, region):
 *     d1<=0 && d2'<=0               -> (0, 0, 1)
 *     d3>=0 && d4<=d3               -> (1, 0, 2)
 *     vc<=0 && d1>=0 && d3<=0       -> (d1/(d1-d3), 0, 4)
 *     d6>=0 && d5<=d6               -> (0, 1, 3)
 *     vb<=0 && d2'>=0 && d6<=0      -> (0, d2'/(d2'-d6), 5)
 *     va<=0 && e1>=0 && e2>=0       -> (1-w, w, 6)   with e1 = d4-d3, e2 = d5-d6, w = e1/(e1+e2)
 *     otherwise the face            -> (vb/s, vc/s, 0) with s = (va+vb)+vc
 *   A quotient whose divisor is 0 is taken as 0; every other quotient is the correctly rounded IEEE one.  Then q = (a + ab*u) + ac*v per component, and q is
 *   CLAMPED INTO THE TRIANGLE'S OWN BOX per axis by comparisons that leave a NaN a NaN: q < lo ? lo : (q > hi ? hi : q), lo / hi the exact min / max of a, b, c.
 *   closest = q, and d2 = (dx*dx + dy*dy) + dz*dz with d = p - q.  u and v are the values the region computed, before the clamp.
 * - The clamp makes pruning exact: with g = max(max(lo-p, p-hi), 0) per axis of a node's box and box_d2 = (gx*gx + gy*gy) + gz*gz, box_d2 <= d2_i holds in
 *   floats for every triangle under the node, so a walk that skips a node iff box_d2 > best returns the definition's answer bit for bit — over any tree whose
 *   boxes contain their vertices, the caller's loose boxes included (DESIGN.md 5.19 has the proof).
 * - A ZERO-AREA TRIANGLE gets what this arithmetic gives: a point of its box, not necessarily its nearest (with a == b the edge-ab region answers a).  The
 *   error is bounded by the triangle's own extent.
 * - INVALID RECORDS AND MISSES.  A record is invalid if a component of point is non-finite, or if max_d2 is NaN or < 0 (-0.0 is 0); that is decided before any
 *   walk.  Invalid records and misses go out as closest = 0, 0, 0, d2 = the bits of max_d2 as given, prim = 0xFFFFFFFF, u = v = 0, region = 0.
 * - The call needs a scene — before any full upload it is RVPT_HIP_ERR_INVALID; the empty scene answers every record with a miss — and no rvpt_hip_set_frame.
 *   dst_bytes must be a multiple of 48, else RVPT_HIP_ERR_INVALID; dst_bytes == 0 is a successful no-op; fewer than 2^32 records per call.
 * - `dst` is host memory or device memory of the context's GPU, classified as for frames.  Device memory must be 16-byte aligned, else RVPT_HIP_ERR_INVALID;
 *   another GPU's memory is RVPT_HIP_ERR_INVALID naming both devices.  In every error case `dst` is untouched.  Host records go through the ray queries' staging
 *   buffer, and only the out fields — the last 32 bytes of a record — travel back; device records never visit the host.
 * - The call is LOCAL: with a communicator it is not collective and touches no peer.
 * - It implies rvpt_hip_wait and leaves untouched the accumulator, rvpt_hip_get_timing, rvpt_hip_get_stats, rvpt_hip_get_launch_info, rvpt_hip_get_cull_info,
 *   the frame counter, and rvpt_hip_last_error on success: a frame dispatched after a point query is bit for bit the frame dispatched without it.
 * - The answer is on the scene as the last update form left it: plain, guarded, sparse, pose or skin.
 * DESIGN.md 5.19 has the kernels and what was measured (profiles/nearest_points.txt).
 *
 * K-NEAREST POINTS — the k nearest triangles of the mesh to the caller's own points, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_NEAREST_POINTS_K(k), records, n * k * sizeof(rvpt_point_hit));      k = 1 .. RVPT_HIP_POINT_MAX_NEAREST
 *
 * `dst` then holds n GROUPS of k consecutive rvpt_point_hit records.  Record 0 of a group carries the point and the bound (point, max_d2); the in fields of
 * records 1 .. k-1 are ignored.  No in field of any record is ever written.  On return the out fields (closest, d2, prim, u, v, region) of record j hold the
 * j-th entry of the group's answer.  The k belongs to the call, not to the record: a launch is uniform in k.  Formats 48 and 57 are the "unknown format" error.
 * - THE ANSWER IS DEFINED WITHOUT REFERENCE TO ANY WALK, as a point query's is.  Every stored triangle i gets the candidate (d2_i, prim_i) of NEAREST POINTS,
 *   by its PER-TRIANGLE ARITHMETIC, unchanged; a candidate whose d2 is NaN is never one.  The answer is the first k, in ascending lexicographic order of
 *   (d2, prim), of all candidates that are smaller than (max_d2, 0xFFFFFFFF).  So d2 == max_d2 is accepted, among equal d2 the smaller reported prim comes
 *   first, and when more than k candidates tie at the k-th distance the smaller numbers are the ones returned.
 * - prim is numbered as a point query numbers it (THE NUMBERING OF prim above): the stored order after an upload, the caller's order after a build form.  The
 *   answer is therefore the same after every builder.
 * - A RADIUS QUERY.  A finite max_d2 makes the form one: the group holds EVERY triangle within the bound if its last slot is a miss, otherwise the k nearest of them.
 * - MISSES AND INVALID RECORDS.  From the first slot no candidate fills, every slot is a miss: closest = 0, 0, 0, d2 = the bits of record 0's max_d2 as given,
 *   prim = 0xFFFFFFFF, u = v = 0, region = 0.  A group whose record 0 is invalid by the rule of NEAREST POINTS gets k such slots, decided before any walk.  The
 *   empty scene answers every group so.
 * - With k = 1 the form is format 4 exactly: RVPT_HIP_FORMAT_NEAREST_POINTS_K(1) is format 4, the same kernels, the same bytes and the same messages.
 * - Each stored triangle is taken to lie under one leaf, as in every tree the library's builders and rvpt_bvh_build make.  A caller's tree that lists a triangle
 *   under two leaves may report it twice.
 * - Everything else is a point query's rule: the call needs a scene and no rvpt_hip_set_frame; dst_bytes must be a multiple of 48 * k, else
 *   RVPT_HIP_ERR_INVALID (the message gives k and the byte count); dst_bytes == 0 is a successful no-op; fewer than 2^32 records (n * k) per call; `dst` is host
 *   memory or 16-byte aligned device memory of the context's GPU, another GPU's memory is an error naming both devices, and in every error case `dst` is
 *   untouched; host records go through the staging buffer and only the out fields travel back; the call is LOCAL under a communicator, implies rvpt_hip_wait,
 *   leaves untouched what a point query leaves untouched, and answers on the scene as the last update form left it.
 * DESIGN.md 5.26 has the kernels and what was measured (profiles/nearest_points_k.txt).
 *
 * BOX OVERLAPS — how many triangles of the mesh meet the caller's own boxes, and which, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_BOX_OVERLAPS, records, n * sizeof(rvpt_box_overlap));
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k), records, n * k * sizeof(rvpt_box_overlap));         k = 1 .. RVPT_HIP_BOX_MAX_GROUP
 *
 * The region form of a query: the broad phase of a collision against the mesh as it is posed or skinned on the device, and the cell test of a conservative
 * (surface) voxelisation.  A record carries a closed box [lo, hi] and a first number prim_from in, and the count and the smallest numbers out.  With
 * RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k), `dst` holds n GROUPS of k consecutive records: record 0 of a group carries the box; the in quads (the first 32 bytes) of
 * records 1 .. k-1 are ignored and never written; the out quad of record j >= 1 is four more prim slots.  A group therefore lists up to S = 4k - 1 numbers:
 * 3, 7, 11 or 15.  The k belongs to the call, not to the record.  RVPT_HIP_FORMAT_BOX_OVERLAPS_K(1) is format 9 itself: the same kernels, bytes and messages.
 * Formats 64 and 69 are the "unknown format" error.
 * - THE ANSWER IS DEFINED WITHOUT REFERENCE TO ANY WALK, as a point query's is.  A is the set of stored triangles that pass THE TEST below and whose reported
 *   number is >= prim_from.  The reported number is a point query's (THE NUMBERING OF prim above): the stored order after an upload, the caller's order after
 *   a build form.  count = |A|.  The prim slots hold the S smallest reported numbers of A in ascending order; from the first slot that A does not fill, every
 *   slot is 0xFFFFFFFF.  The answer is therefore the same on every kind of context, after every builder and on every tree.
 * - PAGING.  If count > S, call again with prim_from = the last listed number + 1: a caller enumerates A in ceil(|A| / S) calls, and count of each call is
 *   what is still to come, the listed ones included.
 * - Each stored triangle is taken to lie under one leaf, as in every tree the library's builders and rvpt_bvh_build make.  A caller's tree that lists a triangle
 *   under two leaves may count it twice.
 * - THE TEST is the separating-axis test of a triangle against a box, 13 axes, in binary32: every product, sum and difference is rounded on its own, no FMA.
 *   Every comparison is a rejection, so a NaN rejects nothing: "min(x, y, z) > r" below stands for x > r and y > r and z > r, "max(x, y, z) < r" likewise.
 *   a, b, c are vert0..2 of the stored row.  A triangle with any non-finite vertex component is never in A.
 *   1. Boxes.  Per axis k, reject if min(a_k, b_k, c_k) > hi_k or max(a_k, b_k, c_k) < lo_k.  Comparisons only.
 *   2. Set-up.  ctr = lo*0.5 + hi*0.5 and h = hi - ctr; v0 = a - ctr, v1 = b - ctr, v2 = c - ctr; e0 = b - a, e1 = c - b, e2 = a - c.
 *   3. Plane.  n = cross(b - a, c - a) with cross(x, y) = (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0), and dot(x, y) = (x0*y0 + x1*y1) + x2*y2.  Per axis,
 *      vmin_k = n_k > 0 ? -h_k - v0_k : h_k - v0_k, and vmax_k is the other choice.  Reject if dot(n, vmin) > 0.  Reject if dot(n, vmax) < 0.
 *   4. Nine edge axes.  For each edge e_i, i = 0, 1, 2, and each axis j = x, y, z, in that nesting order, with k1 = (j + 1) % 3 and k2 = (j + 2) % 3:
 *      p_m = e_i[k1]*v_m[k2] - e_i[k2]*v_m[k1] for m = 0, 1, 2; r = h[k1]*|e_i[k2]| + h[k2]*|e_i[k1]|; reject if min(p0, p1, p2) > r or max(p0, p1, p2) < -r.
 *   The triangle is in A iff nothing rejected.  Touching counts.  A zero-area triangle gets what this arithmetic gives: the segment test for a == b, the box
 *   test alone for a == b == c.
 * - WHAT IS NOT PROMISED.  The test is the ROUNDED form of the separating-axis test: a triangle within rounding of a box face may fall on either side of it.
 *   Where every operation above is exact — small integers, say — the answer is the exact one.
 * - INVALID RECORDS.  A record 0 is invalid if a component of lo or hi is non-finite, or if lo_k > hi_k on some axis; lo == hi is legal, a point or a plane
 *   probe.  Invalidity is decided before any walk: count = 0 and every slot 0xFFFFFFFF.  The empty scene answers every record the same way.
 * - Everything else is a point query's rule: the call needs a scene and no rvpt_hip_set_frame; dst_bytes must be a multiple of 48 * k, else
 *   RVPT_HIP_ERR_INVALID (with k > 1 the message gives k and the byte count); dst_bytes == 0 is a successful no-op; fewer than 2^32 records (n * k) per call;
 *   `dst` is host memory or 16-byte aligned device memory of the context's GPU, another GPU's memory is an error naming both devices, and in every error case
 *   `dst` is untouched; host records go through the staging buffer and only the out quads travel back; the call is LOCAL under a communicator, implies
 *   rvpt_hip_wait, leaves untouched what a point query leaves untouched — a frame dispatched afterwards is bit for bit the frame dispatched without it — and
 *   answers on the scene as the last update form left it: plain, guarded, sparse, pose or skin.
 * DESIGN.md 5.28 has the kernels, why a walk that prunes by step 1 returns exactly A, and what was measured (profiles/box_overlaps.txt).
 *
 * SPHERE SWEEPS — when and where the caller's own moving spheres first touch the mesh, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_SPHERE_SWEEPS, records, n * sizeof(rvpt_sphere_sweep));
 *
 * The sweep form of a query: a character controller's step, a camera boom, a projectile with a size, an object dropped onto the mesh as it is posed or skinned
 * on the device.  `dst` then holds n rvpt_sphere_sweep records: each comes in as a sphere and the motion of its centre (org, radius, dir, tmax) — the centre is
 * org + t*dir for t in [0, tmax], closed; dir need not be a unit vector, so t is in units of dir — and goes out as the first contact (t, prim, u, v), laid out
 * as the out quad of an rvpt_ray_hit.  The in quads are never written.
 * - THE ANSWER IS DEFINED WITHOUT REFERENCE TO ANY WALK, as a point query's is.  Every stored triangle i gets a candidate (t_i, prim_i), or none, by the
 *   arithmetic below; the answer is the lexicographically smallest candidate.  A NaN never wins (no candidate's t is one), and among equal t the smaller
 *   reported prim wins.  The numbering of prim is a ray query's (THE NUMBERING OF prim above): the stored order after an ordinary upload, the caller's order
 *   after a build form.  The answer is therefore the same on every kind of context, after every builder and on every tree.
 * - PER-TRIANGLE ARITHMETIC.  binary32 throughout; every product, sum, quotient and square root is rounded on its own, no FMA; the square root is the
 *   correctly rounded one.  a, b, c = vert0..2 of the stored row; p = org, d = dir, r = radius, T = tmax; dot(x,y) = (x0*y0 + x1*y1) + x2*y2 and
 *   cross(x,y) = (x1*y2 - x2*y1, x2*y0 - x0*y2, x0*y1 - x1*y0).  Per record, once: inv_k = 1/d_k on every axis with d_k != 0, rr = r*r, A = dot(d,d).
 *   Every "max" and "min" below that moves a time is the select written next to it, so that a NaN moves nothing and a zero keeps its sign.
 *   1. OWN BOX.  lo, hi are the exact min / max of a, b, c per axis (fminf / fmaxf; the vertices are finite).  A triangle with a non-finite vertex component
 *      takes no part.  The box is inflated by one rounded operation per side, L = lo - r and H = hi + r.  t_in = 0 and t_out = T; then per axis k:
 *        d_k == 0:  reject if p_k < L_k or p_k > H_k — two comparisons, no arithmetic;
 *        otherwise: t1 = (L_k - p_k)*inv_k, t2 = (H_k - p_k)*inv_k; (near, far) = d_k > 0 ? (t1, t2) : (t2, t1);
 *                   t_in = near > t_in ? near : t_in;   t_out = far < t_out ? far : t_out.
 *      Reject unless t_in <= t_out and t_in < +inf.  A NaN among near and far — 0 * inf from a denormal d_k, or, where the same test runs on a node of a tree,
 *      a node's side that is a NaN — passes neither select and rejects nothing.
 *   2. CONTACT TIME t_tri: the smallest time over seven features, each a number in [0, T] or nothing.  The ROOT of (c0, b0, a0) is
 *      t = c0 / (sqrt(b0*b0 - a0*c0) - b0), taken iff c0 > 0, b0 < 0, a0 > 0, b0*b0 - a0*c0 >= 0, and 0 <= t <= T: the smaller root of a0*t*t + 2*b0*t + c0
 *      for a centre that starts outside and approaches, in the form without cancellation.
 *      For each pair (x0, x1) = (a, b), (b, c), (c, a), with m = p - x0, e = x1 - x0, B = dot(m,d), C = dot(m,m) - rr:
 *        the VERTEX x0:     C <= 0 gives 0; otherwise the ROOT of (C, B, A);
 *        the EDGE x0 -> x1: ee = dot(e,e), md = dot(m,e), nd = dot(d,e); ca = ee*A - nd*nd, cb = ee*B - nd*md, cc = ee*C - md*md (the ray against the infinite
 *                           cylinder, reduced).  Nothing if ee == 0.  cc <= 0 with 0 <= md <= ee (an initial overlap) gives 0; otherwise the ROOT of
 *                           (cc, cb, ca), accepted only where the contact projects into the edge: s = md + t*nd, 0 <= s <= ee.
 *      The FACE: n = cross(b - a, c - a), nn = dot(n,n); nothing if nn is not > 0.  h = dot(p - a, n), rn = r*sqrt(nn), hs = |h|, dn = dot(d,n),
 *        dns = h > 0 ? dn : -dn.  hs <= rn gives the time 0; otherwise, iff hs > rn and dns < 0, the time t = (rn - hs)/dns — the plane pushed out by r*|n|
 *        towards the centre's side — taken iff 0 <= t <= T.  The time is accepted iff closest_point(a, b, c, p + d*t) of NEAREST POINTS — one product and one sum
 *        per component for the centre, then the regions in their order — decides region 0, the face.
 *      Together the seven are the Minkowski sum of the triangle and the ball: a sphere that already overlaps the triangle reports 0.
 *   3. REPORTED TIME.  t_i = t_in > t_tri ? t_in : t_tri, a candidate iff t_tri exists and t_i < +inf.  It is the record's t.  (u, v) is the pair
 *      closest_point(a, b, c, p + d*t_i) computes, before its clamp.  The out quad therefore pipes into an rvpt_surface_point as a point hit's last quad does:
 *      SURFACE POINTS gives the contact point and the stored normal.
 *   4. dir = 0, 0, 0 is a valid record: every axis takes the two comparisons, no ROOT exists (A = 0), and only the candidates at t = 0 remain.
 * - WHY STEP 1 IS THERE: it makes pruning exact, as the clamp does for NEAREST POINTS.  The box of every node above a triangle contains its finite vertices:
 *   node.lo <= lo and node.hi >= hi.  Rounding is monotone, so the inflated node box contains the inflated own box IN FLOATS, and every operation of step 1 is
 *   monotone in L and H.  THE LEMMA: run on the node's box, step 1 passes whenever it passes on the own box, and t_in(node) <= t_in(own) <= t_i.  A walk that
 *   skips a node iff its step 1 rejects or t_in(node) > best — strictly: at equality a smaller prim may still lie below — returns the definition's bytes on any
 *   tree whose boxes contain their vertices, the caller's loose boxes included, in any visiting order (DESIGN.md 5.30 has the proof).
 * - A ZERO-AREA TRIANGLE gets what this arithmetic gives: its face is skipped (nn is 0), its edges and vertices still answer.
 * - WHAT IS NOT PROMISED.  t is the ROUNDED contact time: near a graze the discriminant's cancellation decides between a contact and a miss, and t_in may lift
 *   t above t_tri by the rounding of the own box's slab test.  DESIGN.md 5.30 has the measured distance between the sphere at t and the triangle.
 * - INVALID RECORDS AND MISSES.  A record is invalid if a component of org or dir is non-finite, if radius is NaN, negative or infinite, or if tmax is NaN
 *   or < 0 (-0.0 is 0); that is decided before any walk.  Invalid records and misses go out as t = the bits of tmax as given, prim = 0xFFFFFFFF, u = v = 0.
 * - Everything else is a point query's rule: the call needs a scene — before any full upload it is RVPT_HIP_ERR_INVALID; the empty scene answers every record
 *   with a miss — and no rvpt_hip_set_frame; dst_bytes must be a multiple of 48, else RVPT_HIP_ERR_INVALID; dst_bytes == 0 is a successful no-op; fewer than
 *   2^32 records per call; `dst` is host memory or 16-byte aligned device memory of the context's GPU, another GPU's memory is an error naming both devices,
 *   and in every error case `dst` is untouched; host records go through the staging buffer and only the out quad travels back; the call is LOCAL under a
 *   communicator, implies rvpt_hip_wait, leaves untouched what a point query leaves untouched — a frame dispatched afterwards is bit for bit the frame
 *   dispatched without it — and answers on the scene as the last update form left it: plain, guarded, sparse, pose or skin.
 * DESIGN.md 5.30 has the kernels, the lemma's proof and what was measured (profiles/sphere_sweeps.txt).
 *
 * TRIANGLES — the whole mesh as it now stands:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_TRIANGLES, dst, dst_bytes);
 *
 * `dst` receives n_tris rvpt_triangle rows (64 B each) in the UPDATE ORDER of this context — the order the plain update form takes: the leaf order after an
 * ordinary upload, the caller's own order after a build form or a guarded rebuild.  Row perm[s] of the answer is stored row s.
 * - THE BYTES ARE THE STORED BYTES, all 64 of a row: vert0..vert2 with their w lanes as the last form that wrote them left them, the mat_id row as the last
 *   full upload or build left it.  Nothing is recomputed; a NaN payload in a w lane comes back as it went in.  After a pose or skin update these rows are the
 *   only copy of the moved vertices there is.
 * - ROUND TRIPS.  Passing the answer straight to the plain update form moves nothing.  After a build form, passing it with the stored materials to the same
 *   build count on a fresh context gives the tree a guarded rebuild would give.
 * - `dst` is host memory or device memory of the context's GPU, classified as for frames.  Device memory must be 16-byte aligned, else RVPT_HIP_ERR_INVALID;
 *   another GPU's memory is RVPT_HIP_ERR_INVALID naming both devices.
 * - dst_bytes < n_tris * 64 is RVPT_HIP_ERR_SIZE, and the message gives both numbers.  More is allowed: the bytes past n_tris * 64 are not touched.
 * - Before any full upload the call is RVPT_HIP_ERR_INVALID.  The empty scene is a successful no-op, and `dst` may then be NULL.
 * - In every error case `dst` is untouched.
 * - The call is LOCAL: with a communicator it is not collective and touches no peer.
 * - It implies rvpt_hip_wait, returns after the context's stream has finished writing, and leaves untouched the accumulator, rvpt_hip_get_timing,
 *   rvpt_hip_get_stats, rvpt_hip_get_launch_info, rvpt_hip_get_cull_info, the frame counter, and rvpt_hip_last_error on success: a frame dispatched after the
 *   read is bit for bit the frame dispatched without it.
 *
 * SURFACE POINTS — points on the stored mesh for the (prim, u, v) a query reported, in place:
 *
 *     rvpt_hip_read(ctx, RVPT_HIP_FORMAT_SURFACE_POINTS, records, n * sizeof(rvpt_surface_point));
 *
 * `dst` then holds n rvpt_surface_point records: each comes in as (prim, u, v) and goes out as (point, mat, normal, reserved = 0).  The in fields are never
 * written; flags is reserved and ignored.
 * - prim IS NUMBERED exactly as rvpt_ray_hit::prim and rvpt_point_hit::prim are.  The last float4 of an rvpt_point_hit is already a valid in-quad.
 * - CONVENTION.  u weights vert1 - vert0 and v weights vert2 - vert0: what both query forms report.
 * - ARITHMETIC.  binary32, every operation rounded on its own, no FMA.  a, b, c = vert0..2 of the stored row:
 *     ab = b - a, ac = c - a, point = (a + ab*u) + ac*v per component.
 *   This is the nearest form's q before its clamp: for an rvpt_point_hit the answer equals `closest` wherever the clamp did nothing.  For a ray hit it is NOT
 *   org + t*dir: it is the point of the stored triangle at the reported pair, which differs from the ray's own point by rounding.  (u, v) need not lie in the
 *   triangle: any finite pair is evaluated.
 * - normal is the 12 bytes stored for the hit normal when the row was last written: normalize(cross(vert1 - vert0, vert2 - vert0)) by the cross, dot and
 *   normalize of the frame kernels (the normal intersect_scene normalises, intersection.glsl:511-513), NOT turned towards any ray.  A zero-area triangle gets
 *   what that arithmetic gives.
 * - mat is the stored material index word of the row.
 * - INVALID RECORDS are prim >= n_tris (so 0xFFFFFFFF, a miss piped through, is invalid) or a non-finite u or v.  They go out as point = normal = 0,
 *   mat = 0xFFFFFFFF, reserved = 0.  On the empty scene every record is invalid.
 * - Sizes, alignment, classification, staging, locality, rvpt_hip_wait and what is left alone are a ray query's: dst_bytes a multiple of 48, 0 being a
 *   successful no-op; fewer than 2^32 records per call; device records 16-byte aligned; before any full upload RVPT_HIP_ERR_INVALID; in every error case `dst`
 *   is untouched; for host records only the out fields — the last 32 bytes of a record — travel back.
 * - The answer is on the scene as the last update form left it: a record kept from frame to frame stays attached to the posed or skinned surface.
 * DESIGN.md 5.22 has the kernels and what was measured. */
int rvpt_hip_read(rvpt_hip_ctx *ctx, int format, void *dst, size_t dst_bytes);

/* ---- multi-GPU: one RCCL communicator over the tile_world ranks of a partitioned image (no reference counterpart: the
 * reference is single-device; SURVEY §8(b) "creates streams (+ RCCL comm if n_devices>1)", §8(e)) -------------------
 * The only exchange of the path is the gather above — grouped ncclSend/ncclRecv of each rank's tile-linear accumulator
 * (xGMI: every peer on its own link to the root), nothing per frame.  librccl is loaded on first use.
 *
 * One process per GPU: rank 0 makes an id (comm_unique_id), the host hands the 128 bytes to every rank by whatever
 * means it has (MPI, a file, torch.distributed's store), every rank calls comm_init on its context; rank and world are
 * the context's tile_rank / tile_world.
 * One process, several GPUs: create one context per device (tile_rank i of n, any device ids) and pass them, in rank
 * order, to comm_init_all (ncclCommInitAll); collectives are then driven through rank 0's context alone. */
#define RVPT_HIP_COMM_ID_BYTES 128
int rvpt_hip_comm_unique_id(void *id_out, size_t id_bytes);
int rvpt_hip_comm_init(rvpt_hip_ctx *ctx, const void *unique_id, size_t id_bytes);
int rvpt_hip_comm_init_all(rvpt_hip_ctx *const *ctxs, int n);
/* Collective failure behaviour (ABI 4).  Arguments, allocations and this rank's own frames in flight are dealt with BEFORE a rank
 * enters a group call; a rank that finds its own arguments invalid still takes part in the exchange and reports the error afterwards
 * (it never leaves its peers waiting).  Every collective — and ncclCommInitRank's bootstrap — is given RVPT_HIP_COMM_TIMEOUT_S seconds
 * (default 120): when a peer never arrives the call returns RVPT_HIP_ERR_COMM with the reason in rvpt_hip_last_error, the communicator
 * is aborted and later collectives on the context report "no communicator".  rendering is unaffected.
 *
 * comm_barrier: every rank's work dispatched so far has finished when it returns (rvpt_hip_wait on this rank, then a one-float
 * all-reduce on the communicator: ~30 us warm).  What a host uses to bracket a timed region without a second RCCL communicator of
 * its own (bench.py).  Single-process groups: through rank 0's context. */
int rvpt_hip_comm_barrier(rvpt_hip_ctx *ctx);
/* Leave the communicator (ncclCommDestroy; rvpt_hip_destroy does it too): the context is a plain partition member again, its reads
 * are local.  For hosts whose ranks did not all manage to join.  A single-process group dissolves as a whole. */
int rvpt_hip_comm_destroy(rvpt_hip_ctx *ctx);
/* (ABI 8) What RCCL itself says about the context's communicator — ncclCommCount, ncclCommUserRank, ncclGetVersion (e.g. 22105 = 2.21.5) — so that a
 * scaling record can state that the gather ran over RCCL with N ranks (bench.py: "collective").  RVPT_HIP_ERR_COMM without a communicator; an entry point
 * this RCCL lacks leaves its output 0 / -1.  Any out pointer may be NULL. */
int rvpt_hip_comm_info(rvpt_hip_ctx *ctx, int *n_ranks, int *rank, int *rccl_version);
/* The same gather, leaving the frame on the device: rank 0 passes width*height*16 bytes of its own device memory
 * (row-major RGBA32F); the other ranks pass NULL.  Collective like rvpt_hip_read. */
int rvpt_hip_gather(rvpt_hip_ctx *ctx, void *dst_dev_rgba32f);

/* Multi-GPU plumbing (no reference counterpart; the reference is single-device).
 * tile_buffer: device pointer + byte size of this rank's tile-linear RGBA32F accumulator
 * (owned tiles in ascending slot order, 16x16x4 floats each) — the RCCL gather payload.
 * max_tile_bytes: the same size for the rank that owns most tiles (gather slot size).
 * untile: scatter `n_ranks` gathered slots (device memory, slot r at r*slot_bytes) into a
 * row-major RGBA32F image on this context's device. */
int rvpt_hip_tile_buffer(rvpt_hip_ctx *ctx, void **device_ptr, size_t *bytes,
                         size_t *max_tile_bytes);
int rvpt_hip_untile(rvpt_hip_ctx *ctx, const void *gathered_dev, size_t slot_bytes,
                    uint32_t n_ranks, void *dst_dev_rgba32f);

/* Restore / snapshot the accumulator from host memory (row-major RGBA32F); enables resume of a
 * long accumulation.  (No reference counterpart: its temporal image dies with the process.)
 * `src_rgba32f` may be device memory of the context's GPU (4-byte aligned; classified as for rvpt_hip_read): the tiling kernel reads it directly, the
 * caller guarantees that whatever wrote it has finished.  Device memory of another GPU is RVPT_HIP_ERR_INVALID, naming both devices. */
int rvpt_hip_write_accum(rvpt_hip_ctx *ctx, const void *src_rgba32f, size_t src_bytes);

/* Timing + counters (replaces Timer, src/rvpt/timer.cpp:15-46).  kernel_ms_last: hipEvent time
 * of the last frame-kernel launch; kernel_ms_sum / n_dispatches (launches: a dispatch_frames call is
 * one launch over its n frames) since create or reset. */
int rvpt_hip_get_timing(rvpt_hip_ctx *ctx, float *kernel_ms_last, double *kernel_ms_sum,
                        uint64_t *n_dispatches);
int rvpt_hip_reset_timing(rvpt_hip_ctx *ctx);
/* stats[0] = path segments traced, stats[1] = samples traced (needs RVPT_HIP_COUNT_SEGMENTS). */
int rvpt_hip_get_stats(rvpt_hip_ctx *ctx, uint64_t stats[2]);

/* Launch shape of the last dispatched frame kernel: work-groups, dynamic LDS bytes per work-group,
 * kernel variant (0 brute/LDS-resident with mixed packets, 1 brute/LDS-streamed, 2 bvh: binary per-lane walk, 3 the same with the scene in LDS,
 * 6 brute/LDS-resident packet kernel, 10 bvh over the 4-wide regrouping of the tree, 11 the same with the scene in LDS (and camera packets in the lean
 * configuration); 6, 10 and 11 are the defaults; 4, 5, 7, 8 and 9 were experiments of rounds 3-4, 12 and 13 of round 5, all retired), and how many frames the context
 * keeps in flight (the reference: MAX_FRAMES_IN_FLIGHT = 2, rvpt.h:25).  Any out pointer may be NULL. */
int rvpt_hip_get_launch_info(rvpt_hip_ctx *ctx, uint32_t *grid_blocks, uint32_t *lds_bytes,
                             uint32_t *kernel_variant, uint32_t *frames_in_flight);

/* (ABI 8) Which exact culls of the packet kernel the last dispatched launch rode with: bit 0 = the screen rectangles of the camera rounds,
 * bit 1 = the bounce cull's table (absent when the scene has none or the launch camera is further than 64 scene scales from the origin: the table's premise),
 * bit 2 = the launch's work plan starts every camera round on a 16 x 4 block (where it does not, the kernel skips the rectangles for that round), bit 4 = the leaf
 * boxes of the bounce rounds (with the table; RVPT_HIP_PACKETS_BOX_CULL=0 switches them off), bit 5 = the interleaved claim order (a frame's blocks dealt from all
 * over the frame; RVPT_HIP_PACKETS_INTERLEAVE=0 gives the tile-linear order), bit 6 = the kernel instance for launches with all three culls (the walks without
 * a cull compiled out: fewer registers to keep alive), bit 7 = the batched launch that claims only the blocks that are not sky, bit 8 = the row boxes of bounce
 * packets whose rays leave one triangle (with the leaf boxes; RVPT_HIP_PACKETS_BOX_CULL=0 switches both off), bit 9 = that batched launch
 * (of 16 frames or more) runs each block's frames back to back in groups of 16 and makes the block's camera set-up once per run, bit 10 = the row boxes
 * of bit 8 were made by the tight rule (rvpt_amd/csrc/rvpt_vis.h; always, in this library: the laboratory build can make round 8's tables instead), bit 11 =
 * those packets ride with finite row caps: a round whose rays all rise above their row's cap walks nothing (rvpt_vis.h; always, in this library).  0 for
 * every other kernel.  The image never depends on these; tools/fuzz_culls.py records them. */
int rvpt_hip_get_cull_info(rvpt_hip_ctx *ctx, uint32_t *flags);

const char *rvpt_hip_last_error(rvpt_hip_ctx *ctx);

/* Host-side binned-SAH BVH build with the reference node layout (replaces
 * BinnedBvhBuilder::build_bvh, src/rvpt/bvh_builder.cpp:11-199; called once at init,
 * rvpt.cpp:83-86).  nodes_out must hold 2*n_tris-1 nodes; prim_indices_out n_tris entries
 * (leaf order -> original triangle index, i.e. Bvh::primitive_indices).  No GPU needed. */
int rvpt_bvh_build(const rvpt_triangle *tris, size_t n_tris, rvpt_bvh_node *nodes_out,
                   size_t *n_nodes_out, uint32_t *prim_indices_out);

#ifdef __cplusplus
}
#endif
#endif /* RVPT_HIP_H */
