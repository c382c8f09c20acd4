// rvpt_abi.hip — implementation of the C ABI declared in include/rvpt_hip.h.
//
// Host-side counterpart of the reference seam inside `class RVPT` (src/rvpt/rvpt.cpp): resource
// creation (:639-866), per-frame upload (:96-126), dispatch (:1005-1039, :352-354) and the fence
// (:115-116) become HIP runtime calls on one stream of one device.  No exception leaves this file.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rvpt_hip.h"
#include "../../include/rvpt_hip_lab.h"
#include "rvpt_kernels.h"
#include "bvh_wide.h"
#include "rvpt_refit.h"
#include "rvpt_frames.h"
#include "rvpt_build.h"
#include "rvpt_query.h"
#include "rvpt_nearest.h"
#include "rvpt_surface.h"
#include "rvpt_paths.h"
#include "rvpt_packets.h"
#include "rvpt_math.h"
#include "rvpt_rect.h"
#include "rvpt_vis.h"

#ifndef RVPT_HIP_LAB
#define RVPT_HIP_LAB 0  // 1: the laboratory build (librvpt_hip_debug.so): + the selftests and host-side forms of include/rvpt_hip_lab.h, the opt-in walks, the tuning knobs
#endif
#ifndef RV_REPORT_STACK_OVERFLOW
#define RV_REPORT_STACK_OVERFLOW 0  // (rvpt_device.h) 1: the BVH kernels report a push past the stack the host sized
#endif

// The handful of RCCL (NCCL API) types the gather needs, declared here so that the library BUILDS without the RCCL headers — a
// single-GPU host needs neither header nor library; librccl.so is dlopen()ed when a communicator is first asked for.  Values as in
// rccl.h (NCCL 2.x ABI: ncclFloat32 = 7, ncclSum = 0, a 128-byte unique id).
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef struct {
    char internal[128];
} ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;  // anything else is an error, described by ncclGetErrorString
typedef enum { ncclFloat = 7 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
}

static_assert(rv::kWideChildren == rv::kWideFormChildren && rv::kWideEmpty == rv::kWideFormEmpty, "bvh_wide.h and rvpt_kernels.h describe the same node");
static_assert(sizeof(rvpt_triangle) == 64, "Triangle layout (structs.glsl:1-7)");
static_assert(sizeof(rvpt_bvh_node) == 32, "BvhNode layout (structs.glsl:9-14)");
static_assert(sizeof(rvpt_material) == 48, "Material layout (structs.glsl:22-33)");
static_assert(sizeof(rvpt_render_settings) == 40, "RenderSettings std140 block (compute_pass.comp:28-40)");
static_assert(sizeof(rvpt_camera_data) == 80, "Camera block (compute_pass.comp:44-49)");
static_assert(RVPT_HIP_RAY_MAX_HITS == rv::kQueryMaxHits, "the k of a k-nearest ray query: the header's and the kernels'");
static_assert(sizeof(rvpt_ray_hit) == rv::kQueryRecordBytes && offsetof(rvpt_ray_hit, tmax) == 12 && offsetof(rvpt_ray_hit, dir) == 16 && offsetof(rvpt_ray_hit, flags) == 28 &&
                  offsetof(rvpt_ray_hit, t) == 32 && offsetof(rvpt_ray_hit, prim) == 36 && offsetof(rvpt_ray_hit, u) == 40 && offsetof(rvpt_ray_hit, v) == 44,
              "a ray query's record: three float4 (rvpt_query.hip)");
static_assert(sizeof(rvpt_ray_path) == rv::kPathRecordBytes && offsetof(rvpt_ray_path, seed) == 12 && offsetof(rvpt_ray_path, dir) == 16 && offsetof(rvpt_ray_path, max_bounces) == 28 &&
                  offsetof(rvpt_ray_path, radiance) == 32 && offsetof(rvpt_ray_path, segments) == 44 && RVPT_HIP_PATH_MAX_BOUNCES == rv::kPathMaxBounces,
              "a path query's record: three float4 (rvpt_paths.hip)");
static_assert(sizeof(rvpt_part_move) == 64 && offsetof(rvpt_part_move, first) == 48 && offsetof(rvpt_part_move, count) == 52, "rvpt_part_move: the sixteen words rv::pose_parts reads");
static_assert(sizeof(rvpt_vertex_skin) == 32 && offsetof(rvpt_vertex_skin, weight) == 16 && sizeof(rvpt_bone) == 48 && RVPT_HIP_SKIN_MAX_BONES * sizeof(rvpt_bone) <= 48u * 1024u,
              "rvpt_vertex_skin, rvpt_bone: the two quads and the three quads rv::skin_vertices reads; every matrix fits its 48 KiB of LDS");
static_assert(sizeof(rvpt_ray_path) == sizeof(rvpt_ray_hit) &&offsetof(rvpt_ray_path, radiance) == offsetof(rvpt_ray_hit, t), "ray and path queries share query_records");
static_assert(sizeof(rvpt_point_hit) == rv::kNearestRecordBytes && sizeof(rvpt_point_hit) == sizeof(rvpt_ray_hit) && offsetof(rvpt_point_hit, max_d2) == 12 &&
                  offsetof(rvpt_point_hit, closest) == 16 && offsetof(rvpt_point_hit, d2) == 28 && offsetof(rvpt_point_hit, prim) == 32 && offsetof(rvpt_point_hit, u) == 36 &&
                  offsetof(rvpt_point_hit, v) == 40 && offsetof(rvpt_point_hit, region) == 44,
              "a point query's record: three float4 (rvpt_nearest.hip), and it shares query_records");
static_assert(sizeof(rvpt_surface_point) == rv::kSurfaceRecordBytes && sizeof(rvpt_surface_point) == sizeof(rvpt_ray_hit) && offsetof(rvpt_surface_point, u) == 4 &&
                  offsetof(rvpt_surface_point, v) == 8 && offsetof(rvpt_surface_point, flags) == 12 && offsetof(rvpt_surface_point, point) == 16 &&
                  offsetof(rvpt_surface_point, mat) == 28 && offsetof(rvpt_surface_point, normal) == 32 && offsetof(rvpt_surface_point, reserved) == 44 &&
                  offsetof(rvpt_point_hit, prim) == 32 && offsetof(rvpt_point_hit, u) == 36 && offsetof(rvpt_point_hit, v) == 40 && sizeof(rvpt_triangle) == 64,
              "a surface record: three float4 (rvpt_surface.hip), its in-quad laid out as the last quad of an rvpt_point_hit, and it shares query_records");
static_assert(offsetof(rvpt_triangle, mat_id) == 48 && offsetof(rvpt_bvh_node, bounds) == 8 &&
                  offsetof(rvpt_material, data) == 32 && offsetof(rvpt_render_settings, split_ratio) == 32 &&
                  offsetof(rvpt_camera_data, params) == 64,
              "member offsets");

struct rvpt_hip_ctx {
    int device = 0;
    uint32_t width = 0, height = 0, tiles_x = 0, tiles_y = 0;
    uint32_t tile_rank = 0, tile_world = 1, flags = 0;
    uint32_t n_local_tiles = 0, n_work = 0;
    int num_cus = 0;
    hipStream_t stream = nullptr;            // uploads, blend, read-back — in order
    // frames in flight: frame kernels rotate over `n_slots` streams / sample buffers / counter sets
    // (the reference keeps MAX_FRAMES_IN_FLIGHT = 2 per-frame resource sets, rvpt.h:25)
    static constexpr int kMaxSlots = 8;
    int n_slots = 6;                 // allocated; how many of them a launch rotates over is chosen per launch (slots_for)
    bool slots_fixed = false;        // RVPT_HIP_FRAMES_IN_FLIGHT given: always all of them
    int next_slot = 0;
    bool slot_used[kMaxSlots] = {};  // a launch has gone out on it (its blend_done event means something)
    int last_slots = 0;              // what the last launch rotated over (rvpt_hip_get_launch_info)
    hipStream_t trace_stream[kMaxSlots] = {};
    // Sample buffers: TWO per stream slot, used alternately (round 6).  A launch writes the per-pixel sample means of its frames into one and the blend on the main
    // stream consumes them; with one buffer per slot the slot's NEXT launch had to wait for that blend — trace -> event -> blend -> event -> trace, two cross-stream
    // hand-offs of ~17-20 us each on a 40-us frame (rocprofv3 kernel trace of one frame per launch: profiles/r06_launch_shapes.txt).  With two, the next launch on a
    // stream follows its predecessor in stream order and only waits for the blend of the launch BEFORE that, long finished.
    static constexpr int kBufsPerSlot = 2;
    hipEvent_t trace_done[kMaxSlots] = {}, blend_done[kMaxSlots * kBufsPerSlot] = {};
    rv::SampleRGB *d_samples[kMaxSlots * kBufsPerSlot] = {};  // per-launch sample means awaiting the blend (samples_cap frames each); buffer = slot * 2 + parity
    uint32_t samples_cap[kMaxSlots * kBufsPerSlot] = {};
    bool buf_used[kMaxSlots * kBufsPerSlot] = {};  // a launch has gone out on it (its blend_done event means something)
    int slot_parity[kMaxSlots] = {};
    size_t slot_quads = 0;
    bool overlap = true;
    uint64_t seq = 0;

    float4 *d_tris = nullptr, *d_prep = nullptr, *d_mats = nullptr, *d_nodes = nullptr;
    uint32_t *d_mat_index = nullptr;
    float4 *d_unit_n = nullptr;  // (normalize(n), 0) per triangle (prepare_triangles)
    size_t cap_unit_n = 0;
    size_t n_tris = 0, n_mats = 0, n_nodes = 0;
    uint32_t bvh_height = 0;  // nodes on the longest root-to-leaf path
    // 4-wide form of the same tree (build_wide_nodes; rvpt_bvh4.hip): 128-byte nodes of up to four children, 0 when the tree has no wide form
    float4 *d_wide = nullptr;
    size_t n_wide = 0, cap_wide = 0;
    uint32_t wide_stack_levels = 0;  // most slots a depth-first walk of the wide tree can hold at once
    uint32_t bvh_head_shift = 0;  // see FrameParams::head_shift
    // what a geometry update (upload_scene's update form: same topology, moved vertices) needs from the last full upload: the levels of the breadth-first device
    // layout as index ranges [begin, end) of d_nodes, root level first (at most kBvhStackDepth of them; empty: no tree, or the caller's layout was kept), and the
    // binary node behind every child slot of the wide form (4 words per wide node: build_wide_nodes' kid_map)
    std::vector<std::pair<uint32_t, uint32_t>> refit_levels;
    uint32_t *d_wide_map = nullptr;
    size_t cap_wide_map = 0;
    size_t cap_tris = 0, cap_prep = 0, cap_mat_index = 0, cap_mats = 0, cap_nodes = 0;  // allocated elements
    // the BUILD FORM of upload_scene (rvpt_build.h; build_scene_on_device below): the permutation it sorted the caller's triangles by (perm[j] = caller's index of
    // leaf-order triangle j; have_perm: the stored scene came from a build form, so the update form takes the caller's order), the scratch of the level loops
    // (keys, ranges, flags, offsets: 32 bytes per triangle), rocPRIM's temporary storage, eight counters and their pinned host copy
    uint32_t *d_perm = nullptr;
    size_t cap_perm = 0;
    bool have_perm = false;
    unsigned char *d_build = nullptr, *d_build_temp = nullptr;
    size_t cap_build = 0, cap_build_temp = 0;
    uint32_t *d_build_counters = nullptr, *h_build_words = nullptr;
    // the GUARDED UPDATE of upload_scene (include/rvpt_hip.h): the tree cost's buffer (three result doubles, a gap, then one partial per work-group of
    // rv::tree_cost_partials) and the pinned double it is read into; the cost of the tree the last full upload or build form left (have_cost: there is a level
    // table to compute one by); which builder made the stored tree (0: the caller, an ordinary upload); the caller's materials as they were passed (the device
    // copy's data.w is rewritten by prepare_materials); and the buffer a rebuild's triangles are carried back into, in the caller's order
    double *d_cost = nullptr, *h_cost = nullptr;
    size_t cap_cost = 0;
    double base_cost = 0.0;
    bool have_cost = false;
    enum { kBuiltByCaller = 0, kBuiltLbvh, kBuiltPloc, kBuiltSah };
    int built_by = kBuiltByCaller;
    std::vector<rvpt_material> host_mats;
    float4 *d_carry = nullptr;
    size_t cap_carry = 0;
    // the SPARSE UPDATE of upload_scene (include/rvpt_hip.h): the maps of the stored topology (parent per node, leaf per triangle position; have_sparse_maps:
    // made for the tree in d_nodes, dropped by every full upload, build and rebuild), the inverse of d_perm (have_inv_perm: made for the d_perm of now, dropped
    // whenever that changes), a flag per node (all zero between updates), a claim word per triangle, the words of the validation with their pinned host copy,
    // and the staging buffer of a host source — d_prep holds the live records of the triangles that stay
    uint32_t *d_sparse_parent = nullptr, *d_sparse_leaf_of = nullptr, *d_sparse_dirty = nullptr, *d_sparse_claim = nullptr, *d_inv_perm = nullptr;
    size_t cap_sparse_parent = 0, cap_sparse_leaf_of = 0, cap_sparse_dirty = 0, cap_sparse_claim = 0, cap_inv_perm = 0;
    bool have_sparse_maps = false, have_inv_perm = false;
    uint32_t *d_sparse_words = nullptr, *h_sparse_words = nullptr;
    unsigned char *d_sparse_stage = nullptr;
    size_t cap_sparse_stage = 0;
    // the POSE UPDATE of upload_scene (include/rvpt_hip.h): the REST POSE — the 48 vertex bytes of every stored triangle, in stored order, as the last call of
    // any other form left them.  have_rest: the snapshot belongs to the stored scene; kept by the two pose forms, the two skin forms and the bind (through a guarded rebuild too), dropped by every successful call of another form, taken again by the
    // next pose update.  BVH contexts keep it on the device (three quads per triangle), brute-force contexts on the host (twelve floats per triangle).
    float4 *d_rest = nullptr;
    size_t cap_rest = 0;
    // the GUARDED POSE UPDATE: the rest pose in the caller's order while a rebuild replaces the permutation (allocated at the first such rebuild)
    float4 *d_rest_carry = nullptr;
    size_t cap_rest_carry = 0;
    std::vector<float> h_rest;
    bool have_rest = false;
    // the BIND and the SKIN UPDATE of upload_scene (include/rvpt_hip.h): the binding — three rvpt_vertex_skin records per triangle in the order the plain update
    // form takes — on the device of a BVH context, on the host of a brute-force one; the largest bone index it holds and the smallest record position that
    // holds it; the words of a device list's check with their pinned host copy; and the matrices of the last skin update (BVH contexts: skin_bones of them)
    uint4 *d_skin = nullptr;
    size_t cap_skin = 0;
    std::vector<rvpt_vertex_skin> h_skin;
    bool have_skin = false;
    uint32_t skin_max_bone = 0;
    uint64_t skin_max_pos = 0;
    unsigned long long *d_skin_words = nullptr, *h_skin_words = nullptr;
    float4 *d_bones = nullptr;
    size_t cap_bones = 0;
    uint32_t skin_bones = 0;
    bool have_scene = false;
    // RAY, PATH and POINT QUERIES (rvpt_hip_read with RVPT_HIP_FORMAT_RAY_HITS / RVPT_HIP_FORMAT_RAY_PATHS / RVPT_HIP_FORMAT_NEAREST_POINTS; rvpt_query.h, rvpt_paths.h, rvpt_nearest.h): the staging buffer of host records (bytes) and the launch's scratch — 64 words whose
    // first is the claim counter, then the global part of the traversal stack (words).  Both only grow.  A SURFACE POINTS read stages its host records there
    // too, and a TRIANGLES read into host memory on a context with a permutation scatters its rows into the staging buffer (rvpt_surface.h).
    unsigned char *d_query_stage = nullptr;
    size_t cap_query_stage = 0;
    uint32_t *d_query_scratch = nullptr;
    size_t cap_query_scratch = 0;
    // SURFACE POINTS (rvpt_hip_read with RVPT_HIP_FORMAT_SURFACE_POINTS; rvpt_surface.h): the inverse of d_perm once more, the read side's own — the sparse
    // update's d_inv_perm and its flag belong to the update forms and to the laboratory read-back, which a read must leave as it found them.
    // have_surface_inv: made for the d_perm of now, dropped wherever have_inv_perm is (every full upload, build and rebuild).
    uint32_t *d_surface_inv = nullptr;
    size_t cap_surface_inv = 0;
    bool have_surface_inv = false;

    rvpt_render_settings settings{};
    rvpt_camera_data camera{};
    bool have_frame = false;

    float4 *d_accum = nullptr;
    void *d_rowmajor = nullptr;  // width*height*16 B staging for read / write_accum
    unsigned long long *d_counter = nullptr, *d_stats = nullptr;
    // multi-GPU gather of per-tile radiance: RCCL communicator of the tile_world ranks, rank == tile_rank
    ncclComm_t comm = nullptr;
    hipStream_t comm_stream = nullptr;        // collectives (+ rank 0's un-tiling) run here, never on `stream`: a collective that hangs — a peer that never
                                              // arrives, an abort that fails — leaves rendering, read-back and wait untouched
    bool comm_stream_lost = false;            // a collective timed out on comm_stream: it is abandoned (never waited for, never destroyed)
    float *d_barrier = nullptr;               // one float: the payload of rvpt_hip_comm_barrier's all-reduce
    std::vector<rvpt_hip_ctx *> local_group;  // single-process form (comm_init_all): every rank's context, index == rank
    uint32_t *d_stack_overflow[kMaxSlots] = {};  // HBM-resident BVH kernel: stack levels beyond the LDS ones, per launch in flight
    size_t stack_overflow_cap[kMaxSlots] = {};   // in words
    int debug_checks = 0;                     // RVPT_HIP_DEBUG=1: rvpt_hip_wait reads the kernels' error words (traversal-stack overflow) and fails loudly
    // the bounce cull's table (bounce_visibility, once per upload of a scene the packet kernel can hold): 2 n rows of ceil(n / 32) words
    uint32_t *d_vis = nullptr;
    size_t vis_cap = 0;                       // in words
    float4 *d_leaf_boxes = nullptr;           // the leaf boxes of the bounce rounds (rvpt_vis.h), made with the table; two float4 per kLeafTris triangles
    size_t leaf_boxes_cap = 0;                // in float4
    uint32_t *d_row_bits = nullptr;           // the row boxes of the bounce rounds (rvpt_vis.h), made with the leaf boxes: the refined rows (d_vis' layout) ...
    size_t row_bits_cap = 0;                  // in words
    float4 *d_row_boxes = nullptr;            // ... and every row's own boxes, two float4 per leaf, 32 / kLeafTris * vis_words leaves per row
    size_t row_boxes_cap = 0;                 // in float4
    bool have_row_boxes = false;              // made for the scene in d_prep
    bool row_rule_tight = false;              // ... with the tight rule (rvpt_vis.h: kRowRuleTight; the laboratory build's RVPT_HIP_PACKETS_ROW_RULE=0: round 8's rule)
    uint32_t vis_words = 0;                   // 0: no table for this scene
    double scene_scale = 0.0;                 // largest |coordinate| + largest extent of the uploaded triangles: what float errors of positions scale with
    // screen rectangles of the triangles for the packet kernel's camera rounds (rvpt_rect.h), one buffer per launch slot: rewritten (camera_rects, on the
    // slot's own stream, in front of the frame kernel) only when the camera, the image size or the scene differ from what the slot's buffer was made for
    uint2 *d_rects[kMaxSlots] = {};
    float4 *d_cam_records[kMaxSlots] = {};   // the camera records of the packet kernel (rvpt_early_out.h), made with the slot's rectangles: 16 B per triangle
    size_t rects_cap[kMaxSlots] = {};         // in triangles
    struct RectKey {
        rvpt_camera_data camera;
        uint64_t scene_gen;
    } rects_key[kMaxSlots] = {};
    bool rects_valid[kMaxSlots] = {};
    // the SKY blocks of the slot's camera (rvpt_packets.hip: sky_blocks, sky_list — made with the slot's rectangles, for batched launches): a bit per block, the
    // ascending list of the other blocks and its count, copied into pinned host memory behind them (sky_ready); choose_launch takes the listed path only once it is there
    uint32_t *d_sky_bits[kMaxSlots] = {}, *d_sky_count[kMaxSlots] = {};
    uint2 *d_sky_list[kMaxSlots] = {};       // (block, origin of the block) per entry: rvpt_packets.h, ListedWork::list
    uint32_t *h_sky_count = nullptr;          // kMaxSlots counts (hipHostMalloc)
    hipEvent_t sky_ready[kMaxSlots] = {}, sky_read[kMaxSlots] = {};  // the count has arrived / the last blend that read the slot's sky bits is done
    bool sky_valid[kMaxSlots] = {};           // made for rects_key[slot]
    bool sky_read_used[kMaxSlots] = {};
    uint64_t scene_gen = 0;                  // bumped by every upload_scene
    float4 *d_gather = nullptr;               // rank 0: tile_world slots of slot_quads
    void *d_quant = nullptr;                  // rank 0: width*height*4 B, rgba8 of a gathered frame
    unsigned long long *d_timeline = nullptr;  // RVPT_HIP_TIMELINE=<file>: per-wave timestamps of the last frame
    size_t timeline_words = 0;

    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending, spare;
    float last_ms = 0.f;
    double sum_ms = 0.0;
    uint64_t n_timed = 0;
    uint32_t last_grid = 0, last_lds = 0, last_variant = 0;
    uint32_t last_cull = 0;  // rvpt_hip_get_cull_info: what the last launch rode with
    // The policy knobs, read once at create (read_knobs); the release library reads only the culls' and the interleave's, the others keep these defaults there
    struct Knobs {
        bool bvh_wide = true;             // BVH contexts, lean configuration, reference order: the wide kernels (RVPT_HIP_BVH_PER_LANE / RVPT_HIP_BVH_WIDE=0: binary)
        bool bvh_wide_resident = true;    // RVPT_HIP_BVH_WIDE_RESIDENT=0: LDS-resident scenes on the binary camera-packet kernel instead of the wide tree (trace_bvh4_resident)
        bool bvh_no_resident = false;     // RVPT_HIP_BVH_NO_RESIDENT=1: never the LDS-resident BVH instances
        bool bvh_no_packed_heads = false; // RVPT_HIP_BVH_NO_PACKED_HEADS (set): the stack keeps node indices and the walk fetches (first, count) at the pop (FrameParams::head_shift = 0)
        bool bvh_caller_layout = false;   // RVPT_HIP_BVH_CALLER_LAYOUT (set): the device keeps the uploaded node order (no breadth-first layout, no wide forms)
        bool brute_packets = true;        // LDS-resident brute force, lean configuration: the packet kernel (RVPT_HIP_BRUTE_MIXED_PACKETS / RVPT_HIP_BRUTE_PACKETS=0: trace_brute_resident)
        int force_stack_levels = 0;       // RVPT_HIP_BVH_FORCE_STACK_LEVELS (tests of RVPT_HIP_DEBUG): lie to the kernels about the stack the tree needs
        bool packets_cull = true, packets_bounce_cull = true, packets_box_cull = true;  // RVPT_HIP_PACKETS_CULL / _BOUNCE_CULL / _BOX_CULL=0: each cull off (A/B)
        bool packets_lean_instance = true;  // RVPT_HIP_PACKETS_LEAN_INSTANCE=0: the general instances only (A/B)
        bool packets_row_boxes = true;    // RVPT_HIP_PACKETS_ROW_BOXES=0 (laboratory build): uniform packets walk the union and the shared leaf boxes like the others (A/B)
        int packets_interleave = 1;       // RVPT_HIP_PACKETS_INTERLEAVE=g: launches of < 4 frames deal groups of g (1, 2, 4, 8) blocks from all over the frame; 0 = tile-linear (A/B)
        bool packets_interleave_all = false;  // ... =-g: launches of any size (measured slower for the batched ones: profiles/r06_interleave.txt)
        int packets_sky_list = 1;         // RVPT_HIP_PACKETS_SKY_LIST (laboratory build): batched launches claim only the blocks that are not sky (0 = off, 1 = once the
                                          // slot's list has arrived, 2 = wait for the list on first use: tests/test_sky_list.py)
        int packets_frame_runs = -1;      // RVPT_HIP_PACKETS_FRAME_RUNS (laboratory build): listed launches run each block's frames back to back in groups of this many frames, with the
                                          // camera set-up of a block made once per run (rvpt_packets.h: ListedWork; 0 = frame-major order and per-round set-up, F > 0: groups of F
                                          // for every listed launch; the default: groups of 16 for launches of 16 frames or more — choose_launch)
        std::string timeline_path;        // RVPT_HIP_TIMELINE=<file>: the last frame's per-wave timestamps, written at destroy
        int blocks_per_cu = 0;            // RVPT_HIP_BLOCKS_PER_CU: work-groups per CU of the persistent kernels (0 / -1 here and below: the built-in policy)
        int first_units = 0, claim_units = 0;  // RVPT_HIP_FIRST_UNITS, RVPT_HIP_CLAIM_UNITS: the work plan's static chunk and claim size (plan_work)
        int bvh_refill = 0, bvh_leaf_batch = 0;  // RVPT_HIP_BVH_REFILL, RVPT_HIP_BVH_LEAF_BATCH: FrameParams::bvh_refill, bvh_leaf_batch
        int bvh_top_nodes = -1;           // RVPT_HIP_BVH_TOP_NODES: nodes of the tree's top in LDS (HBM-resident scenes; 0 = no LDS copy)
        int bvh_stack_lds = 0;            // RVPT_HIP_BVH_STACK_LDS: stack levels kept in LDS where the rest goes to global memory
        int bvh_cam_min = 0;              // RVPT_HIP_BVH_CAM_MIN: camera packets: lanes that must start a camera ray together
        int bvh_detach = -1;              // RVPT_HIP_BVH_DETACH: camera packets: the lanes of a node leave the packet at this many or fewer
    } knobs;
    const void *occ_kernel = nullptr;  // cached occupancy query (kernel, lds) -> work-groups per CU
    size_t occ_lds = 0;
    int occ_per_cu = 0;

    std::string err;
};

namespace {

// NOTE: the library does not touch the process environment.  Frames in flight want GPU_MAX_HW_QUEUES >= 8 set by the
// HOST before HIP initialises (include/rvpt_hip.h); rvpt_render, the Python package and bench.py do so.

thread_local std::string g_err;  // for calls that fail before a context exists

// A context's knobs, from its create flags and the environment (rvpt_hip_ctx::Knobs).
rvpt_hip_ctx::Knobs read_knobs(uint32_t flags)
{
    auto set_flag = [](bool &knob, const char *e) { knob = e ? atoi(e) > 0 : knob; };
    auto set_int = [](int &knob, const char *e, int lo, int hi) { knob = e ? std::max(lo, std::min(hi, atoi(e))) : knob; };
    rvpt_hip_ctx::Knobs k;
    k.bvh_wide = (flags & RVPT_HIP_BVH_PER_LANE) == 0;
    k.brute_packets = (flags & RVPT_HIP_BRUTE_MIXED_PACKETS) == 0;
    set_flag(k.packets_cull, getenv("RVPT_HIP_PACKETS_CULL"));
    set_flag(k.packets_bounce_cull, getenv("RVPT_HIP_PACKETS_BOUNCE_CULL"));
    set_flag(k.packets_box_cull, getenv("RVPT_HIP_PACKETS_BOX_CULL"));
    if (const char *e = getenv("RVPT_HIP_PACKETS_INTERLEAVE")) {
        const int g = std::abs(atoi(e));
        k.packets_interleave_all = atoi(e) < 0;
        k.packets_interleave = (g == 1 || g == 2 || g == 4 || g == 8) ? g : 0;
    }
#if RVPT_HIP_LAB
    // Knobs of the laboratory build (librvpt_hip_debug.so, -DRVPT_HIP_LAB=1: rvpt_amd/build.py): the sweeps of rounds 1-5 found each of them flat around its
    // default (profiles/r05_bvh_thresholds.txt, EXPERIMENTS.md), so the release library reads none of them — there they are the constants of the built-in policy.
    set_flag(k.bvh_wide, getenv("RVPT_HIP_BVH_WIDE"));  // experiments: A/B a whole run
    set_flag(k.bvh_wide_resident, getenv("RVPT_HIP_BVH_WIDE_RESIDENT"));
    set_flag(k.bvh_no_resident, getenv("RVPT_HIP_BVH_NO_RESIDENT"));
    k.bvh_no_packed_heads = getenv("RVPT_HIP_BVH_NO_PACKED_HEADS") != nullptr;
    k.bvh_caller_layout = getenv("RVPT_HIP_BVH_CALLER_LAYOUT") != nullptr;
    set_flag(k.brute_packets, getenv("RVPT_HIP_BRUTE_PACKETS"));
    set_int(k.force_stack_levels, getenv("RVPT_HIP_BVH_FORCE_STACK_LEVELS"), 0, INT32_MAX);
    set_flag(k.packets_lean_instance, getenv("RVPT_HIP_PACKETS_LEAN_INSTANCE"));
    set_flag(k.packets_row_boxes, getenv("RVPT_HIP_PACKETS_ROW_BOXES"));
    if (const char *e = getenv("RVPT_HIP_TIMELINE")) k.timeline_path = e;
    set_int(k.blocks_per_cu, getenv("RVPT_HIP_BLOCKS_PER_CU"), 1, 8);
    set_int(k.first_units, getenv("RVPT_HIP_FIRST_UNITS"), 1, 1 << 20);
    set_int(k.claim_units, getenv("RVPT_HIP_CLAIM_UNITS"), 1, 1 << 20);
    set_int(k.bvh_refill, getenv("RVPT_HIP_BVH_REFILL"), 1, 64);
    set_int(k.bvh_leaf_batch, getenv("RVPT_HIP_BVH_LEAF_BATCH"), 1, 64);
    set_int(k.bvh_top_nodes, getenv("RVPT_HIP_BVH_TOP_NODES"), 0, 2048);
    set_int(k.bvh_stack_lds, getenv("RVPT_HIP_BVH_STACK_LDS"), 1, 64);
    set_int(k.bvh_cam_min, getenv("RVPT_HIP_BVH_CAM_MIN"), 1, 65);  // 65 = never
    set_int(k.bvh_detach, getenv("RVPT_HIP_BVH_DETACH"), 0, 64);
    set_int(k.packets_sky_list, getenv("RVPT_HIP_PACKETS_SKY_LIST"), 0, 2);
    set_int(k.packets_frame_runs, getenv("RVPT_HIP_PACKETS_FRAME_RUNS"), 0, 64);
#endif
    return k;
}

void drop_comm(rvpt_hip_ctx *ctx);  // defined with the collective, used by destroy

// RCCL entry points, resolved on first use: a single-GPU host needs no RCCL at all, and inside a torch process the
// already-loaded librccl (same SONAME) is the one that answers
struct Rccl {
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;  // optional
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;     // optional (rvpt_hip_comm_info)
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;  // optional
    ncclResult_t (*GetVersion)(int *) = nullptr;                      // optional
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string why;
};
const Rccl &rccl()
{
    static const Rccl api = [] {
        Rccl r;
        void *h = nullptr;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) {
            r.why = std::string("librccl.so not found: ") + (dlerror() ? dlerror() : "");
            return r;
        }
        auto sym = [&](const char *n) { return dlsym(h, n); };
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
        r.CommInitAll = reinterpret_cast<decltype(r.CommInitAll)>(sym("ncclCommInitAll"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
        r.Send = reinterpret_cast<decltype(r.Send)>(sym("ncclSend"));
        r.Recv = reinterpret_cast<decltype(r.Recv)>(sym("ncclRecv"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
        r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(sym("ncclCommAbort"));
        r.CommCount = reinterpret_cast<decltype(r.CommCount)>(sym("ncclCommCount"));
        r.CommUserRank = reinterpret_cast<decltype(r.CommUserRank)>(sym("ncclCommUserRank"));
        r.GetVersion = reinterpret_cast<decltype(r.GetVersion)>(sym("ncclGetVersion"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
        r.ok = r.GetUniqueId && r.CommInitRank && r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.AllReduce && r.GetErrorString;
        if (!r.ok) r.why = "librccl.so lacks an expected entry point";
        return r;
    }();
    return api;
}

int fail(rvpt_hip_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (ctx ? ctx->err : g_err) = buf;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(ctx, RVPT_HIP_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define RCCL_TRY(ctx, expr)                                                                                       \
    do {                                                                                                          \
        ncclResult_t r_ = (expr);                                                                                 \
        if (r_ != ncclSuccess) return fail(ctx, RVPT_HIP_ERR_COMM, "%s -> %s", #expr, rccl().GetErrorString(r_)); \
    } while (0)

template <typename T>
int grow(rvpt_hip_ctx *ctx, T *&ptr, size_t &cap, size_t need, size_t elem_bytes)
{
    if (need <= cap && ptr) return 0;
    if (ptr) HIP_TRY(ctx, hipFree(ptr));
    ptr = nullptr;
    cap = 0;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ptr), std::max<size_t>(need, 1) * elem_bytes));
    cap = std::max<size_t>(need, 1);
    return 0;
}

int ensure_rowmajor(rvpt_hip_ctx *ctx)
{
    if (!ctx->d_rowmajor) HIP_TRY(ctx, hipMalloc(&ctx->d_rowmajor, static_cast<size_t>(ctx->width) * ctx->height * 16));
    return 0;
}

// fold finished event pairs into the running totals (blocks until they are complete)
int drain_timing(rvpt_hip_ctx *ctx)
{
    for (auto &pr : ctx->pending) {
        HIP_TRY(ctx, hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, pr.first, pr.second));
        ctx->last_ms = ms;
        ctx->sum_ms += ms;
        ctx->n_timed += 1;
        ctx->spare.push_back(pr);
    }
    ctx->pending.clear();
    return 0;
}

// every frame kernel in flight, then everything queued behind them on the main stream
int sync_all(rvpt_hip_ctx *ctx)
{
    for (int i = 0; i < ctx->n_slots; ++i) HIP_TRY(ctx, hipStreamSynchronize(ctx->trace_stream[i]));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

uint32_t owned_tiles(uint32_t n_tiles, uint32_t rank, uint32_t world) { return (n_tiles > rank) ? (n_tiles - rank + world - 1) / world : 0; }

using Kernel = void (*)(const rv::FrameParams);

// The kernel paths of a launch, by the number rvpt_hip_get_launch_info reports (bench.py and the tests compare against these numbers).  Retired: 9, the streamed
// packet kernel of round 4, measured no faster (profiles/r04_exp_stream_packets.patch); 4, 5, the wavefront pipelines of round 3 (profiles/r04_exp_wavefront_pipelines.patch);
// 12, 13, the 8-wide walk and the 4-wide walk over 64-byte quantised nodes of round 5, both bit-exact and measured slower (profiles/r07_exp_bvh8_walk.patch,
// profiles/r07_exp_bvh4_quant_nodes.patch)
enum class Variant : uint32_t {
    BruteResident = 0, BruteStream = 1,  // brute force, scene in LDS (mixed packets: trace_brute_resident) / streamed through LDS
    Bvh = 2, BvhResident = 3,            // binary tree, scene in HBM / in LDS
    BrutePackets = 6,                    // brute force, scene in LDS: the packet kernel (rvpt_packets.hip)
    Wide = 10, WideResident = 11,        // the 4-wide tree (rvpt_bvh4.hip), scene in HBM / in LDS with camera packets
};

// the paths that keep the levels of the traversal stack beyond the LDS ones in global memory (FrameParams::stack_overflow)
bool has_global_stack(Variant v) { return v == Variant::Bvh || v == Variant::Wide || v == Variant::WideResident; }

// rvpt_hip_get_cull_info bits (native.cull_info, tools/fuzz_culls.py): the screen rectangles (FrameParams::rects), the bounce table (vis), camera rounds
// aligned to 16 x 4 blocks, the leaf boxes of the bounce rounds (leaf_boxes), the interleaved claim order (perm_*), the packet instance without the uncull'd walks
// ... and the batched launch that claims only the blocks that are not sky (trace_brute_packets_aa1_culls_listed + blend_accumulate_sky)
// ... and the row boxes of packets that leave one triangle (row_bits, row_boxes)
constexpr uint32_t kCullRects = 1u, kCullBounce = 2u, kCullBlockRounds = 4u, kCullLeafBoxes = 16u, kCullClaimOrder = 32u, kCullLeanInstance = 64u, kCullSkyList = 128u;
constexpr uint32_t kCullRowBoxes = 256u;
constexpr uint32_t kCullFrameRuns = 512u;  // ... and the listed launch in frame-run order with run headers (trace_brute_packets_aa1_culls_listed_runs)
constexpr uint32_t kCullRowRuleTight = 1024u;  // ... and the row boxes it rode with were made by the tight rule (rvpt_vis.h: kRowRuleTight)

struct Launch {
    Kernel kernel;
    Variant variant;
    size_t lds;          // dynamic LDS bytes per work-group
    uint32_t grid;       // work-groups
    uint32_t cull_bits;  // kCull*: kCullRects = the packet kernel's screen rectangles of the triangles ride along (FrameParams::rects)
    bool sky_wanted;     // the lean batched instance with one sample per pixel: the slot's sky list is made for its camera (dispatch_launch)
    bool listed;         // ... and this launch takes the listed path over `work` (kernel = the listed instance)
    rv::ListedWork work;
};

// scene pointers, image geometry, the settings/camera blocks of this frame (compute_pass.comp:28-54)
void fill_frame_params(const rvpt_hip_ctx *ctx, int slot, rv::FrameParams &p, int buf = -1)
{
    const rvpt_render_settings &s = ctx->settings;
    p.tris = ctx->d_tris;
    p.prep = ctx->d_prep;
    p.mat_index = ctx->d_mat_index;
    p.unit_n = ctx->d_unit_n;
    p.mats = ctx->d_mats;
    p.nodes = ctx->d_nodes;
    p.accum = ctx->d_accum;
    p.counter = ctx->d_counter + (ctx->overlap ? slot * rv::kCounterWords : 0);
    p.sample_out = ctx->overlap ? ctx->d_samples[buf >= 0 ? buf : slot * rvpt_hip_ctx::kBufsPerSlot] : nullptr;
    p.stats = (ctx->flags & RVPT_HIP_COUNT_SEGMENTS) ? ctx->d_stats : nullptr;
    p.timeline = nullptr;
    p.n_tris = static_cast<uint32_t>(ctx->n_tris);
    p.n_mats = static_cast<uint32_t>(ctx->n_mats);
    p.n_nodes = static_cast<uint32_t>(ctx->n_nodes);
    p.n_work = ctx->n_work;
    p.n_work_frame = ctx->n_work;
    p.div_work_frame = rv::fast_div_make(ctx->n_work);
    p.div_tiles_x = rv::fast_div_make(ctx->tiles_x);
    p.width = ctx->width;
    p.height = ctx->height;
    p.tiles_x = ctx->tiles_x;
    p.tile_rank = ctx->tile_rank;
    p.tile_world = ctx->tile_world;
    p.frame = s.current_frame;
    p.quantize = (ctx->flags & RVPT_HIP_ACCUM_UNORM8) ? 1u : 0u;
    p.camera_mode = s.camera_mode;
    p.modes[0] = s.top_left_render_mode;
    p.modes[1] = s.top_right_render_mode;
    p.modes[2] = s.bottom_left_render_mode;
    p.modes[3] = s.bottom_right_render_mode;
    p.split_x = s.split_ratio[0];
    p.split_y = s.split_ratio[1];
    p.max_bounces = s.max_bounces;
    p.aa = s.aa;
    p.inv_w = 1.0f / static_cast<float>(ctx->width);  // compute_pass.comp:51
    p.inv_h = 1.0f / static_cast<float>(ctx->height);
    p.cf = static_cast<float>(s.current_frame);                  // :53
    p.inv_cf = 1.0f / static_cast<float>(s.current_frame + 1u);  // :54
    p.aspect = ctx->camera.params[0];
    p.cam_w = 1.0f / rv::tan_det(0.5f * ctx->camera.params[1]);  // camera.glsl:42
    p.ortho_scale = ctx->camera.params[2];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) p.cam[3 * c + r] = ctx->camera.matrix[4 * c + r];
    for (int r = 0; r < 3; ++r) p.cam[9 + r] = ctx->camera.matrix[12 + r];
}

constexpr size_t kLdsBudget = 64 * 1024;  // LDS bytes a work-group gets without opting in to more

// a BVH context with triangles, hence a tree (upload_scene); an empty scene's frames run the brute-force instances over zero triangles
bool is_bvh(const rvpt_hip_ctx *ctx, size_t n_tris) { return (ctx->flags & RVPT_HIP_TRAVERSAL_MASK) != RVPT_HIP_TRAVERSAL_BRUTE && n_tris > 0; }
// the binary walk's stack: at most one push per inner level of the path from the root
uint32_t bvh_stack_levels(const rvpt_hip_ctx *ctx) { return std::max<uint32_t>(1, std::min<uint32_t>(rv::kBvhStackDepth, ctx->bvh_height)); }
size_t stack_lds_bytes(uint32_t levels) { return static_cast<size_t>(levels) * rv::kBlock * 2 * sizeof(uint32_t); }  // a work-group's stack: two words per slot
size_t index_bytes(const rvpt_hip_ctx *ctx) { return ((ctx->n_tris + 3) & ~size_t(3)) * 4; }
size_t bvh_scene_bytes(const rvpt_hip_ctx *ctx) { return ctx->n_nodes * 32 + ctx->n_tris * 64 + index_bytes(ctx) + ctx->n_mats * 48; }

// LDS-resident BVH scenes (nodes + triangles + materials + the whole stack within 64 KiB) run their own kernel instances (unless RVPT_HIP_BVH_NO_RESIDENT)
bool bvh_scene_fits_lds(const rvpt_hip_ctx *ctx)
{
    const size_t bytes = bvh_scene_bytes(ctx);
    return !ctx->knobs.bvh_no_resident && bytes <= rv::kBvhResidentBytes && bytes + stack_lds_bytes(bvh_stack_levels(ctx)) <= kLdsBudget;
}

// How many launches in flight.  Three, except for SHORT launches of the HBM-resident BVH kernel (one frame of a large scene,
// the interactive case: a moving camera leaves nothing to batch): such a launch is mostly ramp-up and tail, and six of them at two
// work-groups per CU overlap those better (tools/archive/sweep_bvh_b1.sh: 1 M-triangle terrain 1080p x 1 spp 4 400 -> 6 180 Msamples/s,
// Cornell 1080p x 4 spp 2 470 -> 2 600; long launches and the LDS-resident kernels: three is as good or better).
int slots_for(const rvpt_hip_ctx *ctx, uint32_t n_frames)
{
    if (!ctx->overlap) return 1;
    if (ctx->slots_fixed) return ctx->n_slots;
    const bool hbm_bvh = is_bvh(ctx, ctx->n_tris) && !bvh_scene_fits_lds(ctx);
    const uint64_t samples = static_cast<uint64_t>(ctx->n_work) * n_frames * static_cast<uint64_t>(std::max(1, ctx->settings.aa));
    const bool short_launch = samples <= 10ull * 1000 * 1000;
    return std::min(ctx->n_slots, (hbm_bvh && short_launch) ? 6 : 3);
}

// every chunk of the work plan is whole 64-item blocks
bool whole_blocks(const rv::FrameParams &p) { return p.first_units % 4u == 0u && p.claim_units % 4u == 0u && p.dyn_base % 4u == 0u && p.shard_len % 4u == 0u; }

// work distribution of the launch (kernels: WavePool): a static first chunk per wave, then sharded claims
// align_units > 1 (the packet kernel: 4 units = the 64 work items of a camera round): chunks start at multiples of it wherever the launch is large enough for
// full-size chunks, so that a camera round is ONE 16 x 4 pixel block (the kernel checks, and skips its rectangle cull for a round that is not)
void plan_work(const rvpt_hip_ctx *ctx, bool regen, rv::FrameParams &p, uint32_t align_units = 1)
{
    p.n_units = p.n_work / rv::kUnit;
    if (!regen) {
        p.first_units = 64 / rv::kUnit;  // 64 pixels per wave, nothing dynamic
        p.claim_units = 1;
    } else {
        // 128-pixel static chunk per wave (less if there is not that much work), 128-pixel claims after that
        p.first_units = std::max(1u, std::min(rv::kMaxClaimUnits, (p.n_units + p.n_waves - 1) / p.n_waves));
        p.claim_units = rv::kMaxClaimUnits;
        // the packet kernel with its culls (round 5) finishes a 64-pixel block of sky in about a microsecond: 128-pixel claims then ask the eight counters for
        // more than they can hand out (one L2 word sustains ~90 atomics per microsecond), and the CLAIMS bound the kernel — 512-pixel claims: 23 979 -> 37 966
        // Msamples/s at the driver's command, 36 169 -> 46 338 over 200 steps; an eighth of the image 0.0164 -> 0.0131 ms per frame; 16 / 32 / 64 counters
        // instead of 8 help only the small claims (tools/archive/r05_claims.sh, profiles/r05_claims.txt)
        if (align_units == 4u) p.claim_units = 32u;
        // (the listed path of round 7 — only the blocks that are not sky, about six claims per wave in 20 frames where there were thirteen — keeps the same rule:
        // 16- and 8-unit claims measured 6 % and 10 % slower, a smaller static chunk within noise: profiles/r07_sky_list.txt)
        // a static chunk of 5-7 units (images of 131-229 k pixels) would start most camera rounds off a block boundary and lose them the rectangles
        if (align_units > 1 && p.first_units > align_units) p.first_units = p.first_units / align_units * align_units;
        if (ctx->knobs.first_units) p.first_units = static_cast<uint32_t>(ctx->knobs.first_units);
        if (ctx->knobs.claim_units) p.claim_units = static_cast<uint32_t>(ctx->knobs.claim_units);
    }
    p.dyn_base = static_cast<uint32_t>(std::min<uint64_t>(p.n_units, static_cast<uint64_t>(p.first_units) * p.n_waves));
    p.shard_len = (p.n_units - p.dyn_base + rv::kClaimShards - 1) / rv::kClaimShards;
    if (align_units > 1) p.shard_len = (p.shard_len + align_units - 1) / align_units * align_units;  // (the kernel clips a shard at n_units)
}

// The packet kernel's claim order over a frame's blocks (FrameParams::perm_*): only when every chunk of the plan is whole blocks (so that a camera round is one
// block of the order), the frame is whole groups, and the products of the map stay inside 32 bits.  Launches of fewer than four frames only: a wave of a one-frame
// launch holds its static chunk and ONE or two 512-item claims, which in tile-linear order are all sky or all model — the waves on the sky leave at 45 us, those on
// the model at 80-115 (profiles/r06_interleave.txt); dealt from all over the frame every claim costs about the same and the launch is 14 % shorter (one frame per
// launch 38 300 -> 42 300 Msamples/s).  A 20-frame launch gives every wave thirteen claims, which even out by themselves: there the order measured 2-4 % slower.
// (the ctx-free core: rvpt_claim_order of the laboratory build walks it without a GPU)
bool plan_claim_order(const uint32_t n_work_frame, const uint32_t g, uint32_t &groups_out, uint32_t &stride_out, uint32_t &shift_out)
{
    if (g == 0 || (g & (g - 1u)) != 0u || g > 8u) return false;
    const uint32_t blocks = n_work_frame / 64u;
    if (n_work_frame % (64u * g) || blocks / g < 16u) return false;
    const uint32_t groups = blocks / g;
    // the stride: nearest below the golden section of `groups` that is coprime to it (consecutive multiples of it mod `groups` are a low-discrepancy sequence:
    // any run of the order samples the frame evenly)
    auto gcd = [](uint32_t a, uint32_t b) {
        while (b) {
            const uint32_t t = a % b;
            a = b;
            b = t;
        }
        return a;
    };
    // ... = groups / (k + 0.618...) for the smallest k = 1, 2, ... that keeps (group index) * stride inside 32 bits: k = 1 up to ~82 000 groups (1920 x 1080 has
    // 32 640 blocks), a 3840 x 2160 frame takes k = 4; beyond k = 16 (frames of more than ~17 M pixels) the order stays tile-linear
    const uint64_t room = 0xFFFFFFFFull / groups;
    uint32_t stride = 0;
    for (uint32_t k = 1; k <= 16u && stride == 0u; ++k) {
        const uint32_t want = static_cast<uint32_t>(groups / (k + 0.6180339887498949));
        if (want <= room) stride = want;
    }
    while (stride > 1u && gcd(stride, groups) != 1u) stride -= 1u;
    if (stride <= 1u) return false;
    uint32_t shift = 0;
    while ((1u << shift) < g) shift += 1;
    groups_out = groups;
    stride_out = stride;
    shift_out = shift;
    return true;
}

void plan_interleave(const rvpt_hip_ctx *ctx, rv::FrameParams &p)
{
    p.perm_groups = 0;
    p.perm_stride = 1;
    p.perm_shift = 0;
    p.div_perm_groups = rv::fast_div_make(1);
    const uint32_t g = static_cast<uint32_t>(ctx->knobs.packets_interleave);
    if (g == 0 || !whole_blocks(p)) return;
    if (!ctx->knobs.packets_interleave_all && p.n_work >= 4u * p.n_work_frame) return;
    uint32_t groups, stride, shift;
    if (!plan_claim_order(p.n_work_frame, g, groups, stride, shift)) return;
    p.perm_groups = groups;
    p.perm_stride = stride;
    p.perm_shift = shift;
    p.div_perm_groups = rv::fast_div_make(groups);
}

// The whole decision for one launch: the kernel path, its LDS and FrameParams, the grid, the work plan and the culls.  `p` comes filled by
// fill_frame_params, with p.n_work the launch's work items; `lone`: nothing of this context is in flight; `slots`: launches in flight (slots_for); `slot`: this launch's.
int choose_launch(rvpt_hip_ctx *ctx, rv::FrameParams &p, bool lone, int slots, int slot, Launch &l)
{
    const rvpt_hip_ctx::Knobs &k = ctx->knobs;
    const bool bvh = is_bvh(ctx, ctx->n_tris);  // no tree = empty scene
    const bool ordered = bvh && (ctx->flags & RVPT_HIP_TRAVERSAL_MASK) == RVPT_HIP_TRAVERSAL_BVH_ORDERED;
    const bool regen = (ctx->flags & RVPT_HIP_KERNEL_SIMPLE) == 0;  // persistent work-groups (KERNEL_SIMPLE: one pixel per lane, one wave per 64 pixels)
    // the lean kernels cover the default configuration (Kajiya everywhere, pinhole); anything else runs the GENERIC ones
    const bool generic = p.camera_mode != 0 || p.modes[0] != 9 || p.modes[1] != 9 || p.modes[2] != 9 || p.modes[3] != 9;
    p.head_shift = k.bvh_no_packed_heads ? 0u : ctx->bvh_head_shift;

    // 1. The path.
    // brute force keeps the whole scene in LDS when it fits the 64 KiB a work-group gets without opting in to more
    const size_t resident_bytes = ctx->n_tris * 64 + index_bytes(ctx) + (ctx->n_mats <= rv::kResidentMaxMats ? ctx->n_mats * 48 : 0) +
                                  (rv::kBlock / 64) * 64 * sizeof(uint32_t);
    const bool resident = ctx->n_tris <= rv::kResidentMaxTris && resident_bytes <= kLdsBudget;
    // the packet form of the resident brute-force kernel (rvpt_packets.hip): full packets of one kind per round, camera rays with the
    // packet-uniform early-out; the lean configuration only
    // (one sample per pixel — the headline's configuration — has an instance of its own: 15-word queue entries, six work-groups per CU instead of five)
    const size_t packets_bytes = ctx->n_tris * 64 + index_bytes(ctx) + ctx->n_mats * 48 +
                                 (rv::kBlock / 64) * (p.aa == 1 ? rv::kPacketQueueWordsAA1 : rv::kPacketQueueWords) * 64 * sizeof(uint32_t);
    const bool packets = resident && ctx->n_tris > 0 && !generic && regen && p.max_bounces >= 1 && p.max_bounces <= 1023 && p.aa <= 1023 &&
                         ctx->n_mats <= rv::kResidentMaxMats && k.brute_packets && packets_bytes <= kLdsBudget;
    const bool bvh_resident = bvh && bvh_scene_fits_lds(ctx);
    // the 4-wide form of the tree (rvpt_bvh4.hip): lean configuration, reference order; half the dependent steps per ray
    const bool wide = bvh && !ordered && regen && ctx->n_wide > 0 && k.bvh_wide && p.head_shift != 0;
    // ... and its LDS-resident instance, with camera packets over the wide nodes: every wide node, the prepared triangles, material indices and materials
    // beside FOUR stack levels (the rest of a lane's stack in its global column: a work-group then takes 27 KB for the default scene and five fit a CU;
    // with eight levels 22 700, with four 25 100 Msamples/s; with camera packets 26 100-26 350 against the binary camera-packet kernel's 23 100:
    // tools/archive/ab_wide_resident.sh, profiles/r04_ab_wide_resident.txt)
    const uint32_t wr_levels_want = k.bvh_stack_lds > 0 ? static_cast<uint32_t>(k.bvh_stack_lds) : 4u;
    auto wide_resident_bytes = [&](uint32_t levels) { return stack_lds_bytes(levels) + 2 * sizeof(float4) + ctx->n_wide * rv::kWideTopQuads * 16 + ctx->n_tris * 64 + index_bytes(ctx) + ctx->n_mats * 48; };
    const Variant v = l.variant = !bvh ? (packets ? Variant::BrutePackets : resident ? Variant::BruteResident : Variant::BruteStream)
                                : bvh_resident ? (wide && k.bvh_wide_resident && wide_resident_bytes(wr_levels_want) <= kLdsBudget ? Variant::WideResident : Variant::BvhResident)
                                : wide ? Variant::Wide : Variant::Bvh;
    // 2. Its LDS and FrameParams.
    // BVH: traversal stack sized from the tree.  HBM-resident scenes keep only the first stack levels in LDS (the rest overflows to global memory, rarely
    // touched) so that the top of the tree fits beside them at full occupancy; LDS-resident scenes keep the whole stack
    const uint32_t lds_levels_want = k.bvh_stack_lds > 0 ? static_cast<uint32_t>(k.bvh_stack_lds) : 8u;
    p.stack_levels = bvh_stack_levels(ctx);
    p.stack_lds_levels = bvh_resident ? p.stack_levels : std::min(p.stack_levels, lds_levels_want);
    // short LDS-resident traversals: let the whole packet finish before refilling (64); long HBM traversals: refill once
    // half of the packet waits, run the parked leaves in batches of 16 lanes, 3 work-groups per CU (swept on the Cornell and
    // 1M-triangle scenes, both traversal orders, frames dispatched in batches: profiles/r01_bvh_knob_sweeps.txt)
    p.bvh_refill = k.bvh_refill ? static_cast<uint32_t>(k.bvh_refill) : (bvh_resident ? 64u : 32u);
    p.bvh_leaf_batch = k.bvh_leaf_batch ? static_cast<uint32_t>(k.bvh_leaf_batch) : 16u;
    // top of the tree in LDS (HBM-resident scenes): 256 nodes = 8 KiB by default (with 8 two-word stack levels in LDS: 24 KiB per
    // work-group, six per CU — what the registers allow anyway; swept: tools/archive/sweep_bvh_top.sh, profiles/r02_sweeps.txt), never more than the tree has (even count: sibling pairs)
    const uint32_t top_want = k.bvh_top_nodes >= 0 ? static_cast<uint32_t>(k.bvh_top_nodes) : 256u;
    p.bvh_top_nodes = (bvh && !bvh_resident) ? std::max(2u, std::min<uint32_t>(top_want, static_cast<uint32_t>(ctx->n_nodes)) & ~1u) : 0u;  // at least the root's line
    // camera packets (trace_bvh4_resident: lanes that start camera rays together walk the tree as one wave-uniform packet in the reference's fixed child
    // order): at least bvh_cam_min lanes must start a camera ray at once; the lanes of a node leave the packet when at most bvh_detach of them are in it
    // (LDS-resident scenes: nobody leaves measured best; the binary-tree form of round 4, +5 % resident / +-0 HBM-resident, is profiles/r04_exp_campack_binary.patch)
    p.bvh_cam_min = k.bvh_cam_min ? static_cast<uint32_t>(k.bvh_cam_min) : 24u;
    p.bvh_detach = k.bvh_detach >= 0 ? static_cast<uint32_t>(k.bvh_detach) : 0u;
    const int sel = (regen ? 0 : 1) | (generic ? 2 : 0);
    bool cull = false;  // packet kernel: the screen rectangles of the triangles ride along
    if (v == Variant::BruteResident || v == Variant::BruteStream) {
        static const Kernel kernels[2][4] = {  // [streamed][sel]
            {rv::trace_brute_resident<true, false>, rv::trace_brute_resident<false, false>, rv::trace_brute_resident<true, true>, rv::trace_brute_resident<false, true>},
            {rv::trace_brute_stream<true, false>, rv::trace_brute_stream<false, false>, rv::trace_brute_stream<true, true>, rv::trace_brute_stream<false, true>}};
        l.kernel = kernels[v == Variant::BruteStream ? 1 : 0][sel];
        l.lds = v == Variant::BruteResident ? resident_bytes : static_cast<size_t>(rv::kBlock / 64) * (rv::kStreamDepth * rv::kWaveChunk * 64 + 64 * sizeof(uint32_t));
    } else if (v == Variant::Bvh || v == Variant::BvhResident) {
        static const Kernel kernels[2][2][4] = {  // [ordered][resident][sel]
            {{rv::trace_bvh<true, false, false, false>, rv::trace_bvh<false, false, false, false>, rv::trace_bvh<true, false, true, false>, rv::trace_bvh<false, false, true, false>},
             {rv::trace_bvh<true, true, false, false>, rv::trace_bvh<false, true, false, false>, rv::trace_bvh<true, true, true, false>, rv::trace_bvh<false, true, true, false>}},
            {{rv::trace_bvh<true, false, false, true>, rv::trace_bvh<false, false, false, true>, rv::trace_bvh<true, false, true, true>, rv::trace_bvh<false, false, true, true>},
             {rv::trace_bvh<true, true, false, true>, rv::trace_bvh<false, true, false, true>, rv::trace_bvh<true, true, true, true>, rv::trace_bvh<false, true, true, true>}}};
        l.kernel = kernels[ordered ? 1 : 0][bvh_resident ? 1 : 0][sel];
        l.lds = stack_lds_bytes(p.stack_lds_levels) + (bvh_resident ? bvh_scene_bytes(ctx) : static_cast<size_t>(p.bvh_top_nodes) * 32);
    } else if (v == Variant::Wide) {
        l.kernel = generic ? rv::trace_bvh4_generic : rv::trace_bvh4;
        p.wide = ctx->d_wide;
        p.n_wide = static_cast<uint32_t>(ctx->n_wide);
        p.stack_levels = std::max<uint32_t>(1, ctx->wide_stack_levels);
        p.stack_lds_levels = std::min(p.stack_levels, lds_levels_want);
        // one node in the LDS copy of the tree top, and how many by default: 8 KiB, as the binary kernel's 256 nodes
        const uint32_t node_bytes = rv::kWideTopQuads * 16u;
        const uint32_t wide_top_want = k.bvh_top_nodes >= 0 ? static_cast<uint32_t>(k.bvh_top_nodes) : 64u;
        // (the knob counts NODES, and a wide node is four binary ones: whatever it asks for, the stack levels + the root record + the top nodes stay within
        // the 64 KiB a work-group can have — ADVICE r4: RVPT_HIP_BVH_TOP_NODES=2048 used to ask for 256 KiB and fail at launch)
        const size_t fixed = stack_lds_bytes(p.stack_lds_levels) + 2 * sizeof(float4);
        const uint32_t wide_top_fit = static_cast<uint32_t>((kLdsBudget - std::min(fixed, kLdsBudget)) / node_bytes);
        p.wide_top_nodes = std::min<uint32_t>({wide_top_want, p.n_wide, wide_top_fit});
        l.lds = fixed + static_cast<size_t>(p.wide_top_nodes) * node_bytes;
    } else if (v == Variant::WideResident) {
        l.kernel = generic ? rv::trace_bvh4_resident_generic : rv::trace_bvh4_resident;
        p.wide = ctx->d_wide;
        p.n_wide = static_cast<uint32_t>(ctx->n_wide);
        p.wide_top_nodes = p.n_wide;
        p.stack_levels = std::max<uint32_t>(1, ctx->wide_stack_levels);
        p.stack_lds_levels = std::min(p.stack_levels, wr_levels_want);
        l.lds = wide_resident_bytes(p.stack_lds_levels);
    } else {  // Variant::BrutePackets
        l.kernel = (p.aa == 1) ? rv::trace_brute_packets_aa1 : rv::trace_brute_packets;
        // + the screen rectangles (8 B per triangle, padded to 16) when they fit beside the rest
        const size_t rect_bytes = ((ctx->n_tris + 1) & ~size_t(1)) * 8;
        cull = k.packets_cull && packets_bytes + rect_bytes <= kLdsBudget;
        l.lds = packets_bytes + (cull ? rect_bytes : 0);
        // the bounce cull's premise: positions carry float errors of at most 2^-13 of the scene's scale — true while the camera (the origin of the first
        // segment) is no further than 64 scene scales from the world origin (rvpt_packets.hip: bounce_visibility)
        const float *o = ctx->camera.matrix + 12;
        const double far = rv::kBounceCameraScales * ctx->scene_scale;
        if (k.packets_bounce_cull && ctx->vis_words > 0 && std::fabs(o[0]) <= far && std::fabs(o[1]) <= far && std::fabs(o[2]) <= far) {
            p.vis = ctx->d_vis;
            p.vis_words = ctx->vis_words;
            p.vis_stride = (ctx->vis_words + 3u) & ~3u;
            if (k.packets_box_cull && ctx->d_leaf_boxes) p.leaf_boxes = ctx->d_leaf_boxes;
            if (p.leaf_boxes && k.packets_row_boxes && ctx->have_row_boxes) p.row_bits = ctx->d_row_bits, p.row_boxes = ctx->d_row_boxes;
        }
    }
    if (bvh && k.force_stack_levels > 0) {  // tests: a stack smaller than the tree needs — the kernels clamp and report (RVPT_HIP_DEBUG)
        p.stack_levels = static_cast<uint32_t>(k.force_stack_levels);
        p.stack_lds_levels = std::min(p.stack_lds_levels, p.stack_levels);
    }
    // 3. The grid, from the occupancy of the general instance of the path.
    const uint32_t blocks_needed = (p.n_work + rv::kBlock - 1) / rv::kBlock;
    l.grid = blocks_needed;  // one-pixel-per-lane kernel: one wave per 64 pixels
    if (regen) {             // persistent work-groups
        if (ctx->occ_kernel != reinterpret_cast<const void *>(l.kernel) || ctx->occ_lds != l.lds) {
            int q = 0;
            HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, reinterpret_cast<const void *>(l.kernel), rv::kBlock, l.lds));
            ctx->occ_kernel = reinterpret_cast<const void *>(l.kernel);
            ctx->occ_lds = l.lds;
            ctx->occ_per_cu = q;
        }
        const int occ = std::max(1, std::min(ctx->occ_per_cu, 8));
        // With frames overlapped in flight a frame kernel takes only 2 work-groups per CU: the kernels of consecutive
        // frames then co-reside (2 + 2 waves per SIMD) and a frame's tail hides under the next frame's body (swept on
        // MI355X: profiles/README.md).  The HBM-resident BVH kernels take 3-4 per CU: the register file holds 7 waves
        // per SIMD in all, so the kernels of the frames in flight fill the CU between them either way, and larger
        // per-group shares balance better (swept: profiles/r01_bvh_knob_sweeps.txt).
        // (LDS-resident BVH with several frames per launch: 3 measured 6 % better than 2; one frame per launch: 2.)
        // Brute force with several frames per launch (>= 4): a launch is long against its own ramp-up and drain, so it takes
        // the register file's five work-groups per CU and consecutive launches overlap only at their ends (swept on MI355X,
        // tools/archive/sweep_batch_bpc.sh: 8 frames per launch x 5 per CU = 6 080 / 6 500 Msamples/s over 20 / 200 frames against
        // 5 670 / 6 410 for one frame per launch x 2 per CU x 3 launches in flight).
        const bool batched = p.n_work >= 4 * p.n_work_frame;
        const bool hbm_bvh = bvh && !bvh_resident;
        const int small_per_cu = batched ? (bvh ? 3 : 8) : 2;  // (brute force, batched: what LDS and registers allow — five work-groups per CU, six for the aa == 1 instance)
        int per_cu = ctx->overlap ? std::min(occ, hbm_bvh ? (slots > 3 ? 2 : 3) : small_per_cu) : occ;
        // ... which assumes that launches overlap.  A LONE launch of the HBM-resident BVH kernel — nothing of this context in flight when it goes
        // out: a rank's 20-step share sent as one launch, the first launch of a burst — has nobody to share the CU with and takes what the registers
        // allow (six per CU): rank 2's share of an 8-way partition as one 20-frame launch, C4 geometry 0.132 -> 0.079 ms per frame, C3 0.675 -> 0.519
        // (tools/archive/sweep_share_shapes.sh, profiles/r04_share_shapes.txt); launches that follow while it runs keep the overlapping shape
        // Only launches of >= 16 frames: a caller that sends such a launch has batched what it had; the first of a stream of SMALLER launches must
        // leave room for the next (measured: C3 at 8 frames per launch 3 240 -> 3 110 Msamples/s when the first launch took the whole CU).
        if (ctx->overlap && hbm_bvh && lone && p.n_work >= 16u * p.n_work_frame) per_cu = occ;
        if (k.blocks_per_cu) per_cu = k.blocks_per_cu;  // (RVPT_HIP_BLOCKS_PER_CU: instead of all of the above)
        l.grid = std::min<uint32_t>(blocks_needed, static_cast<uint32_t>(ctx->num_cus) * static_cast<uint32_t>(per_cu));
    }
    p.n_waves = l.grid * (rv::kBlock / 64);
    // 4. The work plan (the packet kernel: camera rounds of whole 16 x 4 blocks) and the packet kernel's claim order.
    plan_work(ctx, regen, p, v == Variant::BrutePackets ? 4u : 1u);
    if (v == Variant::BrutePackets) plan_interleave(ctx, p);
    // 5. The lean packet instances, for launches with all three culls on and every chunk of the plan whole blocks (the default for a scene with a table): no
    // uncull'd walks — fewer registers to keep alive (SGPR spills 54 -> 19 for one sample per pixel when measured in round 6, 22 with today's compiler, 20 for the listed instance; every spill is a v_readlane / v_writelane the VALU issues) —
    // with or without the interleaved claim order of short launches (its scalars cost the batched launches' kernel eleven spills more).  LAST, because it depends
    // on the work plan (whole_blocks), which depends on the grid (p.n_waves); the grid is the general instance's, which needs no fewer resources (tests/test_abi_exports.py).
    const bool lean = v == Variant::BrutePackets && cull && p.vis && p.leaf_boxes && p.sample_out && whole_blocks(p) && k.packets_lean_instance;
    if (lean)
        l.kernel = p.perm_groups != 0u ? ((p.aa == 1) ? rv::trace_brute_packets_aa1_culls_order : rv::trace_brute_packets_culls_order)
                                       : ((p.aa == 1) ? rv::trace_brute_packets_aa1_culls : rv::trace_brute_packets_culls);
    // 6. The listed path (round 7): a batched launch of the lean one-sample instance whose camera leaves SKY blocks — no triangle's rectangle holds them, so their camera
    // round walks nothing, every ray misses and the path ends there — claims only the other blocks; blend_accumulate_sky makes the sky's samples from the RNG.  Only
    // with the slot's list for THIS camera already on the host (a moving camera, the first launch after a camera or scene change: the path above), never waited for.
    l.sky_wanted = lean && p.aa == 1 && p.perm_groups == 0u && p.n_work >= 4u * p.n_work_frame && k.packets_sky_list > 0;
    l.listed = false;
    uint32_t n_listed = 0;
    if (l.sky_wanted && ctx->sky_valid[slot] && ctx->rects_valid[slot] && std::memcmp(&ctx->rects_key[slot].camera, &ctx->camera, sizeof(ctx->camera)) == 0 &&
        ctx->rects_key[slot].scene_gen == ctx->scene_gen) {
        const hipError_t arrived = hipEventQuery(ctx->sky_ready[slot]);
        if (arrived == hipErrorNotReady) (void)hipGetLastError();  // (an answer, not an error)
        if (arrived == hipSuccess) {
            const uint32_t n_blocks = p.n_work_frame / 64u;
            n_listed = ctx->h_sky_count[slot];
            if (n_listed < n_blocks && n_listed > 0u) {
                const uint32_t n_work = p.n_work;
                p.n_work = p.n_work / p.n_work_frame * n_listed * 64u;
                plan_work(ctx, regen, p, 4u);
                l.listed = whole_blocks(p);  // (a list too short for whole-block chunks: the path above)
                if (!l.listed) {
                    p.n_work = n_work;
                    plan_work(ctx, regen, p, 4u);
                }
            }
        }
    }
    if (l.listed) {
        l.kernel = nullptr;  // (dispatch_launch launches the listed instance)
        l.work.list = ctx->d_sky_list[slot];
        l.work.n_listed_frame = 64u * n_listed;
        l.work.div_listed_frame = rv::fast_div_make(64u * n_listed);
        // Frame runs (the origin of a block is two 16-bit fields of the list's entry).  Groups of 16 frames, for launches that hold a whole group: measured on the
        // headline (profiles/frame_runs.txt), 200 steps as 4 x 50 frames gain 3 % at F = 4, 8 and 16 alike, but a lone 20-frame launch LOSES 3 % at F = 8 — where a
        // 512-item claim is exactly one block's run, eight camera rounds of one block in one wave — and nothing at 4 (two blocks per claim) or 16 (a run is two
        // claims).  Shorter launches keep the frame-major order.
        const uint32_t n_frames = p.n_work / (64u * n_listed);
        const uint32_t run_frames = k.packets_frame_runs >= 0 ? static_cast<uint32_t>(k.packets_frame_runs) : (n_frames >= 16u ? 16u : 0u);
        rv::listed_runs_make(l.work, n_listed, n_frames, (p.width <= 65536u && p.height <= 65536u) ? run_frames : 0u);
    }
    l.cull_bits = (cull ? kCullRects : 0u) | (p.vis ? kCullBounce : 0u) | ((v == Variant::BrutePackets && p.first_units % 4u == 0u) ? kCullBlockRounds : 0u) |
                  (p.leaf_boxes ? kCullLeafBoxes : 0u) | (p.perm_groups != 0u ? kCullClaimOrder : 0u) | (lean ? kCullLeanInstance : 0u) | (l.listed ? kCullSkyList : 0u) |
                  (p.row_boxes ? kCullRowBoxes : 0u) | ((l.listed && l.work.run_frames != 0u) ? kCullFrameRuns : 0u) |
                  ((p.row_boxes && ctx->row_rule_tight) ? kCullRowRuleTight : 0u);
    return 0;
}

}  // namespace

extern "C" {

int rvpt_hip_abi_version(void) { return RVPT_HIP_ABI_VERSION; }

uint32_t rvpt_hip_build_flags(void) { return (RVPT_HIP_LAB ? RVPT_HIP_BUILD_LAB : 0u) | (RV_REPORT_STACK_OVERFLOW ? RVPT_HIP_BUILD_DEBUG_CHECKS : 0u); }

int rvpt_hip_device_count(int *count)
{
    if (!count) return fail(nullptr, RVPT_HIP_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(nullptr, RVPT_HIP_ERR_NO_DEVICE, "hipGetDeviceCount -> %s", hipGetErrorString(e));
    }
    *count = n;
    return RVPT_HIP_OK;
}

int rvpt_hip_create(rvpt_hip_ctx **out, int device_id, uint32_t width, uint32_t height, uint32_t tile_rank,
                    uint32_t tile_world, uint32_t flags)
{
    if (!out) return fail(nullptr, RVPT_HIP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (width == 0 || height == 0 || tile_world == 0 || tile_rank >= tile_world)
        return fail(nullptr, RVPT_HIP_ERR_INVALID, "bad geometry %ux%u rank %u/%u", width, height, tile_rank, tile_world);
    if (static_cast<uint64_t>(width) * height > 0x7FFFFFFFull) return fail(nullptr, RVPT_HIP_ERR_INVALID, "image too large");
    if ((flags & RVPT_HIP_TRAVERSAL_MASK) == RVPT_HIP_TRAVERSAL_MASK) return fail(nullptr, RVPT_HIP_ERR_INVALID, "unknown traversal mode in flags");
    if (flags & ~static_cast<uint32_t>(RVPT_HIP_FLAGS_KNOWN))
        return fail(nullptr, RVPT_HIP_ERR_INVALID, "unknown bits 0x%x in flags (0x40 / 0x80 / 0x100 were the wavefront pipelines of ABI 3-4, retired in ABI 5)", flags & ~static_cast<uint32_t>(RVPT_HIP_FLAGS_KNOWN));
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return fail(nullptr, RVPT_HIP_ERR_NO_DEVICE, "no HIP device visible");
    if (device_id < 0 || device_id >= n_dev) return fail(nullptr, RVPT_HIP_ERR_INVALID, "device %d out of range (%d devices)", device_id, n_dev);

    {  // one line, once per process: the seven streams of a context want eight hardware queues (include/rvpt_hip.h, PROCESS ENVIRONMENT)
        static bool noted = false;
        const char *q = getenv("GPU_MAX_HW_QUEUES");
        if (!noted && !getenv("RVPT_HIP_QUIET") && (!q || atoi(q) < 8)) {
            noted = true;
            std::fprintf(stderr, "[rvpt_hip] note: GPU_MAX_HW_QUEUES is %s; launches in flight share hardware queues below 8 (measured -10 %%). "
                                 "Set GPU_MAX_HW_QUEUES=8 before the first HIP call of the process (RVPT_HIP_QUIET=1 silences this note).\n", q ? q : "unset");
        }
    }
    rvpt_hip_ctx *ctx = new (std::nothrow) rvpt_hip_ctx;
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_HIP, "out of host memory");
    ctx->device = device_id;
    ctx->width = width;
    ctx->height = height;
    ctx->tiles_x = (width + RVPT_HIP_TILE - 1) / RVPT_HIP_TILE;
    ctx->tiles_y = (height + RVPT_HIP_TILE - 1) / RVPT_HIP_TILE;
    ctx->tile_rank = tile_rank;
    ctx->tile_world = tile_world;
    ctx->flags = flags;
    ctx->timing = (flags & RVPT_HIP_TIMING) != 0;
    ctx->n_local_tiles = owned_tiles(ctx->tiles_x * ctx->tiles_y, tile_rank, tile_world);
    ctx->n_work = ctx->n_local_tiles * 256u;

    auto bail = [&](int code) {
        std::string keep = ctx->err;
        rvpt_hip_destroy(ctx);
        g_err = keep;
        return code;
    };
#define CREATE_TRY(expr)                                                                                      \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            fail(ctx, RVPT_HIP_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_));                            \
            return bail(RVPT_HIP_ERR_HIP);                                                                    \
        }                                                                                                     \
    } while (0)
    CREATE_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    CREATE_TRY(hipGetDeviceProperties(&prop, device_id));
    ctx->num_cus = prop.multiProcessorCount;
    CREATE_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    // every rank allocates the largest slot (rank 0's) so that the gather payload has one size
    const size_t slot_quads = std::max<size_t>(static_cast<size_t>(owned_tiles(ctx->tiles_x * ctx->tiles_y, 0, tile_world)) * 256u, 1);
    ctx->slot_quads = slot_quads;
    CREATE_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_accum), slot_quads * sizeof(float4)));
    CREATE_TRY(hipMemsetAsync(ctx->d_accum, 0, slot_quads * sizeof(float4), ctx->stream));
    if (const char *e = getenv("RVPT_HIP_FRAMES_IN_FLIGHT")) {
        ctx->n_slots = std::max(1, std::min(atoi(e), int(rvpt_hip_ctx::kMaxSlots)));
        ctx->slots_fixed = true;
    }
    ctx->overlap = ctx->n_slots > 1 && getenv("RVPT_HIP_NO_OVERLAP") == nullptr;
    if (!ctx->overlap) ctx->n_slots = 1;
    CREATE_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_counter), ctx->n_slots * rv::kCounterWords * sizeof(unsigned long long)));
    CREATE_TRY(hipMemsetAsync(ctx->d_counter, 0, ctx->n_slots * rv::kCounterWords * sizeof(unsigned long long), ctx->stream));
    for (int i = 0; i < ctx->n_slots; ++i) {
        CREATE_TRY(hipStreamCreateWithFlags(&ctx->trace_stream[i], hipStreamNonBlocking));
        CREATE_TRY(hipEventCreateWithFlags(&ctx->trace_done[i], hipEventDisableTiming));
        for (int b = i * rvpt_hip_ctx::kBufsPerSlot; b < (i + 1) * rvpt_hip_ctx::kBufsPerSlot; ++b) {
            CREATE_TRY(hipEventCreateWithFlags(&ctx->blend_done[b], hipEventDisableTiming));
            if (ctx->overlap) {
                CREATE_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_samples[b]), slot_quads * sizeof(rv::SampleRGB)));
                CREATE_TRY(hipMemsetAsync(ctx->d_samples[b], 0, slot_quads * sizeof(rv::SampleRGB), ctx->stream));
                ctx->samples_cap[b] = 1;
            }
        }
    }
    ctx->knobs = read_knobs(flags);
    if (const char *e = getenv("RVPT_HIP_DEBUG")) ctx->debug_checks = atoi(e) > 0 ? 1 : 0;
    if (ctx->debug_checks && !RV_REPORT_STACK_OVERFLOW) {  // never a silent no-op: the release kernels only clamp, nothing would ever set the word
        fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "RVPT_HIP_DEBUG=1 needs the kernels' internal checks, which this build of the library does not carry "
                                            "(rvpt_hip_build_flags() bit 1): load librvpt_hip_debug.so");
        return bail(RVPT_HIP_ERR_UNSUPPORTED);
    }
    CREATE_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_stats), rv::kStatStripes * rv::kStatStride * sizeof(unsigned long long)));
    CREATE_TRY(hipMemsetAsync(ctx->d_stats, 0, rv::kStatStripes * rv::kStatStride * sizeof(unsigned long long), ctx->stream));
    CREATE_TRY(hipStreamSynchronize(ctx->stream));
#undef CREATE_TRY
    *out = ctx;
    return RVPT_HIP_OK;
}

void rvpt_hip_destroy(rvpt_hip_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    drop_comm(ctx);
    for (int i = 0; i < rvpt_hip_ctx::kMaxSlots; ++i)
        if (ctx->d_stack_overflow[i]) (void)hipFree(ctx->d_stack_overflow[i]);
    if (ctx->comm_stream && !ctx->comm_stream_lost) (void)hipStreamDestroy(ctx->comm_stream);  // (a lost one still holds a collective that never completes)
    for (int i = 0; i < rvpt_hip_ctx::kMaxSlots; ++i) {
        if (ctx->d_rects[i]) (void)hipFree(ctx->d_rects[i]);
        if (ctx->d_cam_records[i]) (void)hipFree(ctx->d_cam_records[i]);
    }
    if (ctx->d_vis) (void)hipFree(ctx->d_vis);
    if (ctx->d_leaf_boxes) (void)hipFree(ctx->d_leaf_boxes);
    if (ctx->d_row_bits) (void)hipFree(ctx->d_row_bits);
    if (ctx->d_row_boxes) (void)hipFree(ctx->d_row_boxes);
    if (ctx->d_gather) (void)hipFree(ctx->d_gather);
    if (ctx->d_barrier) (void)hipFree(ctx->d_barrier);
    if (ctx->d_quant) (void)hipFree(ctx->d_quant);
    for (int i = 0; i < rvpt_hip_ctx::kMaxSlots; ++i)
        if (ctx->trace_stream[i]) (void)hipStreamSynchronize(ctx->trace_stream[i]);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < rvpt_hip_ctx::kMaxSlots; ++i) {  // (after the drain: a blend_accumulate_sky on the main stream reads the bits)
        if (ctx->d_sky_bits[i]) (void)hipFree(ctx->d_sky_bits[i]);
        if (ctx->d_sky_list[i]) (void)hipFree(ctx->d_sky_list[i]);
        if (ctx->d_sky_count[i]) (void)hipFree(ctx->d_sky_count[i]);
        if (ctx->sky_ready[i]) (void)hipEventDestroy(ctx->sky_ready[i]);
        if (ctx->sky_read[i]) (void)hipEventDestroy(ctx->sky_read[i]);
    }
    if (ctx->h_sky_count) (void)hipHostFree(ctx->h_sky_count);
    if (ctx->h_build_words) (void)hipHostFree(ctx->h_build_words);
    if (ctx->h_cost) (void)hipHostFree(ctx->h_cost);
    if (ctx->h_sparse_words) (void)hipHostFree(ctx->h_sparse_words);
    if (ctx->h_skin_words) (void)hipHostFree(ctx->h_skin_words);
    if (ctx->d_timeline && !ctx->knobs.timeline_path.empty()) {  // debugging aid: dump the last frame's wave timeline
        std::vector<unsigned long long> h(ctx->timeline_words);
        if (hipMemcpy(h.data(), ctx->d_timeline, ctx->timeline_words * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE *f = fopen(ctx->knobs.timeline_path.c_str(), "wb")) {
                fwrite(h.data(), 8, h.size(), f);
                fclose(f);
            }
        }
        (void)hipFree(ctx->d_timeline);
    }
    for (auto &pr : ctx->pending) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    for (auto &pr : ctx->spare) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    for (int i = 0; i < rvpt_hip_ctx::kMaxSlots; ++i) {
        if (ctx->trace_stream[i]) (void)hipStreamSynchronize(ctx->trace_stream[i]);
        if (ctx->trace_done[i]) (void)hipEventDestroy(ctx->trace_done[i]);
        for (int b = i * rvpt_hip_ctx::kBufsPerSlot; b < (i + 1) * rvpt_hip_ctx::kBufsPerSlot; ++b) {
            if (ctx->blend_done[b]) (void)hipEventDestroy(ctx->blend_done[b]);
            if (ctx->d_samples[b]) (void)hipFree(ctx->d_samples[b]);
        }
        if (ctx->trace_stream[i]) (void)hipStreamDestroy(ctx->trace_stream[i]);
    }
    void *bufs[] = {ctx->d_tris, ctx->d_prep, ctx->d_mats, ctx->d_nodes, ctx->d_wide, ctx->d_wide_map, ctx->d_mat_index, ctx->d_unit_n, ctx->d_accum,
                    ctx->d_rowmajor, ctx->d_counter, ctx->d_stats, ctx->d_perm, ctx->d_build, ctx->d_build_temp, ctx->d_build_counters, ctx->d_cost, ctx->d_carry,
                    ctx->d_sparse_parent, ctx->d_sparse_leaf_of, ctx->d_sparse_dirty, ctx->d_sparse_claim, ctx->d_inv_perm, ctx->d_sparse_words, ctx->d_sparse_stage,
                    ctx->d_query_stage, ctx->d_query_scratch, ctx->d_surface_inv, ctx->d_rest, ctx->d_rest_carry, ctx->d_skin, ctx->d_skin_words, ctx->d_bones};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

namespace {

// What upload_scene derives from the vertex positions in d_tris, shared by the full upload and the geometry update.
// The prepared records, the material indices and the hit normals of the n_tris triangles in d_tris (on ctx->stream, behind the copy that filled d_tris):
static int launch_prepare_triangles(rvpt_hip_ctx *ctx, size_t n_tris)
{
    if (n_tris == 0) return 0;
    const uint32_t n = static_cast<uint32_t>(n_tris);
    hipLaunchKernelGGL(rv::prepare_triangles, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_tris, n, ctx->d_prep, ctx->d_mat_index, ctx->d_unit_n);
    HIP_TRY(ctx, hipGetLastError());
    return 0;
}

// ... and the bounce cull's table with its scene scale and leaf boxes, for scenes the packet kernel can hold (brute-force contexts, <= kResidentMaxTris triangles);
// `tris` is the caller's HOST array (only its vertices are read), d_prep already holds its prepared records
static int derive_bounce_state(rvpt_hip_ctx *ctx, bool bvh, const rvpt_triangle *tris, size_t n_tris)
{
    int rc;
    ctx->vis_words = 0;
    ctx->scene_scale = 0.0;
    ctx->have_row_boxes = false;
    if (!bvh && n_tris > 0 && n_tris <= rv::kResidentMaxTris) {
        const double scale = rv::bounce_scene_scale(reinterpret_cast<const float *>(tris), n_tris);
        if (scale > 0.0) {
            const uint32_t n = static_cast<uint32_t>(n_tris), words = (n + 31u) / 32u;
            const uint32_t stride = (words + 3u) & ~3u;  // rows 16-byte aligned and a multiple of four words apart: a bounce round loads four words of a lane's row at once
            const size_t total = static_cast<size_t>(2) * n * stride;
            if ((rc = grow(ctx, ctx->d_vis, ctx->vis_cap, total, sizeof(uint32_t)))) return rc;
            hipLaunchKernelGGL(rv::bounce_visibility, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_prep, n, rv::kBounceMarginScales * scale, words,
                               stride, ctx->d_vis);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->vis_words = words;
            ctx->scene_scale = scale;
            // ... and the leaf boxes of the same triangles (host arithmetic on the caller's array; rvpt_vis.h)
            // (a whole word's boxes — 32 / kLeafTris of them — are requested together: the array is padded to whole words, the padding's triangles do not exist)
            const size_t n_leaves = static_cast<size_t>(words) * (32u / rv::kLeafTris);
            std::vector<float> boxes(8 * n_leaves, 0.0f);
            rv::bounce_leaf_boxes(reinterpret_cast<const float *>(tris), n_tris, scale, boxes.data());
            if ((rc = grow(ctx, ctx->d_leaf_boxes, ctx->leaf_boxes_cap, 2 * n_leaves, sizeof(float4)))) return rc;
            HIP_TRY(ctx, hipMemcpy(ctx->d_leaf_boxes, boxes.data(), boxes.size() * sizeof(float), hipMemcpyHostToDevice));
            // ... and the row boxes (rvpt_vis.h): every row's refined words and its own box per leaf, from the records and the leaf boxes just copied
            if ((rc = grow(ctx, ctx->d_row_bits, ctx->row_bits_cap, total, sizeof(uint32_t)))) return rc;
            if ((rc = grow(ctx, ctx->d_row_boxes, ctx->row_boxes_cap, static_cast<size_t>(2) * n * 2 * n_leaves, sizeof(float4)))) return rc;
            bool tight = true;
#if RVPT_HIP_LAB
            if (const char *e = getenv("RVPT_HIP_PACKETS_ROW_RULE")) tight = atoi(e) > 0;  // read at every upload: 0 = the tables of round 8's rule (A/B, bit-exactness)
#endif
            hipLaunchKernelGGL(rv::bounce_row_boxes, dim3(static_cast<uint32_t>((total + 63) / 64)), dim3(64), 0, ctx->stream, ctx->d_prep, n, scale, words, stride,
                               reinterpret_cast<const float *>(ctx->d_leaf_boxes), ctx->d_row_bits, reinterpret_cast<float *>(ctx->d_row_boxes), tight ? 1u : 0u);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->have_row_boxes = true;
            ctx->row_rule_tight = tight;
        }
    }
    return 0;
}

// is `p` device memory (hipMalloc: a torch tensor's storage, say)?  Plain host memory is unknown to the runtime, which answers with an error and keeps it as
// the thread's last error: cleared here.  Pinned and managed memory can be read on the host and count as host memory.
static bool is_device_pointer(const void *p)
{
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}

// The frame pointer of rvpt_hip_read / rvpt_hip_write_accum (`what`: "dst" / "src"): host memory, or device memory of the context's GPU, which the layout kernels
// then write or read in place.  Device memory of another GPU and device memory that is not 4-byte aligned are refused before anything touches them.
static int classify_frame_pointer(rvpt_hip_ctx *ctx, const void *p, const char *what, bool *device)
{
    *device = is_device_pointer(p);
    if (!*device) return RVPT_HIP_OK;
    hipPointerAttribute_t attr{};
    HIP_TRY(ctx, hipPointerGetAttributes(&attr, p));
    if (attr.device != ctx->device)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "%s is device memory of GPU %d, the context lives on GPU %d: a frame stays on the context's own device", what, attr.device, ctx->device);
    if (reinterpret_cast<uintptr_t>(p) % 4u)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "%s is device memory at %p: a frame on the device needs 4-byte alignment", what, p);
    return RVPT_HIP_OK;
}

// The cost of the tree in d_nodes (rvpt_refit.hip: two kernels on ctx->stream, then one double read behind them).  Needs the level table: the end of its last
// level is the end of the tree in the breadth-first device layout.  Without one (no tree, or the laboratory's caller-layout knob) the cost is 0 and
// *have is false.
static int device_tree_cost(rvpt_hip_ctx *ctx, double *cost, bool *have)
{
    *cost = 0.0, *have = false;
    if (ctx->refit_levels.empty()) return RVPT_HIP_OK;
    const uint32_t n_nodes = static_cast<uint32_t>(std::min<size_t>(ctx->n_nodes, ctx->refit_levels.back().second));
    if (n_nodes == 0) return RVPT_HIP_OK;
    const uint32_t n_partials = (n_nodes + rv::kTreeCostBlock - 1u) / rv::kTreeCostBlock;
    if (int rc = grow(ctx, ctx->d_cost, ctx->cap_cost, static_cast<size_t>(n_partials) + 4u, sizeof(double))) return rc;
    if (!ctx->h_cost) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_cost), sizeof(double)));
    double *const partials = ctx->d_cost + 4;
    hipLaunchKernelGGL(rv::tree_cost_partials, dim3(n_partials), dim3(rv::kTreeCostBlock), 0, ctx->stream, ctx->d_nodes, n_nodes, partials);
    hipLaunchKernelGGL(rv::tree_cost_finish, dim3(1), dim3(rv::kTreeCostBlock), 0, ctx->stream, partials, n_partials, ctx->d_nodes, ctx->d_cost);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cost, ctx->d_cost, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *cost = ctx->h_cost[0], *have = true;
    return RVPT_HIP_OK;
}

// The update form of rvpt_hip_upload_scene (include/rvpt_hip.h): same triangle count and tree topology as the last full upload, new vertex positions.  Takes the
// twelve floats vert0..vert2 of every triangle (the stored mat_id rows, the materials and the tree's (first, count) words stay) and recomputes what depends on
// positions: prepared records and hit normals, the boxes of the binary nodes (level by level, deepest first) and their copies in the wide nodes, the bounce
// cull's table, scale and leaf boxes.  What depends on topology alone — bvh_height, bvh_head_shift, n_wide, wide_stack_levels, hence the launch choice — stays.
static int update_geometry_tail(rvpt_hip_ctx *ctx, bool bvh, const rvpt_triangle *tris, size_t n_tris);

static int update_geometry(rvpt_hip_ctx *ctx, const rvpt_triangle *tris, size_t n_tris)
{
    if (!ctx->have_scene)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "geometry update (no nodes, no materials) before any full upload_scene on this context: there is no scene to update");
    if (n_tris != ctx->n_tris)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "geometry update with %zu triangles, the uploaded scene has %zu: a full upload_scene changes the count", n_tris, ctx->n_tris);
    const bool bvh = is_bvh(ctx, n_tris);
    if (bvh && ctx->refit_levels.empty())  // (the laboratory's knob only: the release library always makes the breadth-first layout and names no laboratory knob)
#if RVPT_HIP_LAB
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the breadth-first device layout of the tree: RVPT_HIP_BVH_CALLER_LAYOUT keeps the caller's, which has no level ranges");
#else
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the level ranges of the tree's device layout, which this context does not hold");
#endif
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!bvh && is_device_pointer(tris))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "geometry update of a brute-force context from a device pointer: its scene scale and leaf boxes are computed on the host, pass a host array");
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight finish on the old geometry
    // 48 of every 64 bytes: the mat_id row of d_tris stays (no index to validate); the source may be host or device memory
    if (ctx->have_perm) {  // the stored scene came from a build form: `tris` are in the CALLER'S order and go through the permutation the build kept
        const float4 *src = reinterpret_cast<const float4 *>(tris);
        if (!is_device_pointer(tris)) {  // staged in d_prep, which prepare_triangles rewrites below
            HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_prep, sizeof(rvpt_triangle), tris, sizeof(rvpt_triangle), offsetof(rvpt_triangle, mat_id), n_tris, hipMemcpyHostToDevice, ctx->stream));
            src = ctx->d_prep;
        }
        HIP_TRY(ctx, rv::build_gather_vertices(ctx->stream, src, ctx->d_perm, static_cast<uint32_t>(n_tris), ctx->d_tris));
    } else {
        HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_tris, sizeof(rvpt_triangle), tris, sizeof(rvpt_triangle), offsetof(rvpt_triangle, mat_id), n_tris, hipMemcpyDefault, ctx->stream));
    }
    return update_geometry_tail(ctx, bvh, tris, n_tris);
}

// ... and what follows once d_tris holds the moved vertices, shared with the skin update, whose kernel writes them: prepared records and hit normals, every
// box of the tree, the wide copies, the bounce cull's state.  `tris`: the caller's host array on brute-force contexts, unread on BVH contexts.
static int update_geometry_tail(rvpt_hip_ctx *ctx, bool bvh, const rvpt_triangle *tris, size_t n_tris)
{
    if (int rc = launch_prepare_triangles(ctx, n_tris)) return rc;
    if (bvh) {
        const uint32_t n_nodes = static_cast<uint32_t>(ctx->n_nodes);
        for (size_t l = ctx->refit_levels.size(); l-- > 0;) {
            const auto [begin, end] = ctx->refit_levels[l];
            hipLaunchKernelGGL(rv::refit_level, dim3((end - begin + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_nodes, begin, end, n_nodes, ctx->d_tris, static_cast<uint32_t>(n_tris));
        }
        if (ctx->n_wide) {
            const uint32_t n_slots = static_cast<uint32_t>(ctx->n_wide * 4);
            hipLaunchKernelGGL(rv::refit_wide_gather, dim3((n_slots + 255u) / 256u), dim3(256), 0, ctx->stream, reinterpret_cast<float *>(ctx->d_wide), ctx->d_wide_map, n_slots,
                               ctx->d_nodes, n_nodes);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // caller may free its array on return
    if (int rc = derive_bounce_state(ctx, bvh, tris, n_tris)) return rc;
    ctx->scene_gen += 1;  // the slots' screen rectangles and sky lists belong to the old geometry
    return RVPT_HIP_OK;
}

// The BUILD FORM of rvpt_hip_upload_scene (include/rvpt_hip.h; BVH contexts): triangles in the caller's order and materials, no nodes — the tree is built on
// the device (rvpt_build.h: the specification of the tree and the stages).  It is born in the breadth-first layout the full upload makes on the host, with its
// level table, its height and its 4-wide form; the host reads one word per level.  `tris` may be host memory or device memory of the context's GPU.
// `ploc`: the PLOC tree (RVPT_HIP_NODES_BUILD_PLOC) instead of the LBVH between stage 3 and stage 5, with the fallback rule of rvpt_build.h.
// `sah`: the SAH tree (RVPT_HIP_NODES_BUILD_SAH) in place of stages 1 - 4: the order of stage 3 is the index array its level loop leaves.
static int build_scene_on_device(rvpt_hip_ctx *ctx, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t n_mats, bool ploc, bool sah)
{
    int rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n = static_cast<uint32_t>(n_tris);
    const bool device_source = is_device_pointer(tris);
    size_t cap_counters = ctx->d_build_counters ? rv::kBuildCounters : 0;
    if ((rc = grow(ctx, ctx->d_build_counters, cap_counters, rv::kBuildCounters, sizeof(uint32_t)))) return rc;
    if (!ctx->h_build_words) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_build_words), rv::kBuildCounters * sizeof(uint32_t)));
    uint32_t *const h = ctx->h_build_words;
    auto read_word = [&](uint32_t &out, const uint32_t *dev) {  // one word behind everything queued on the stream
        hipError_t e = hipMemcpyAsync(h, dev, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        out = h[0];
        return e;
    };
    // materials[int(mat_id.x)] must stay inside the buffer: validated BEFORE anything of the stored scene is touched, on the host or by a kernel
    if (!device_source) {
        for (size_t i = 0; i < n_tris; ++i) {
            const float m = tris[i].mat_id[0];
            if (!(m >= 0.0f) || static_cast<size_t>(static_cast<int>(m)) >= n_mats)
                return fail(ctx, RVPT_HIP_ERR_INVALID, "triangle %zu: material index %g outside [0,%zu)", i, static_cast<double>(m), n_mats);
        }
    } else {
        uint32_t bad = 0;
        HIP_TRY(ctx, rv::build_validate_materials(ctx->stream, reinterpret_cast<const float4 *>(tris), n, static_cast<uint32_t>(std::min<size_t>(n_mats, 0x80000000u)), ctx->d_build_counters));
        HIP_TRY(ctx, read_word(bad, ctx->d_build_counters + rv::kBuildFirstBad));
        if (bad != 0xFFFFFFFFu) {
            float m = 0.0f;
            HIP_TRY(ctx, hipMemcpy(&m, &tris[bad].mat_id[0], sizeof m, hipMemcpyDeviceToHost));
            return fail(ctx, RVPT_HIP_ERR_INVALID, "triangle %zu: material index %g outside [0,%zu)", static_cast<size_t>(bad), static_cast<double>(m), n_mats);
        }
    }
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight still read the old scene
    // scratch of the level loops, in bytes per region: keys / ranges A / wide heads (8 n), sorted keys / wide heads (8 n), ranges B / the two wide queues (8 n),
    // then three arrays of n + 1 words (flags A, flags B, offsets)
    const size_t words = ((static_cast<size_t>(n) + 1u) * 4u + 15u) & ~size_t(15);
    const size_t lbvh_bytes = 24u * static_cast<size_t>(n) + 3u * words;  // (a multiple of 8: the PLOC regions behind it hold 8-byte pairs)
    const size_t scratch_bytes = sah ? std::max(lbvh_bytes, rv::sah_scratch_bytes(n)) : lbvh_bytes + (ploc ? rv::ploc_scratch_bytes(n) : 0u);
    size_t temp_bytes = 0;
    HIP_TRY(ctx, rv::build_temp_bytes(n, &temp_bytes));
    if (sah) {
        size_t sah_bytes = 0;
        HIP_TRY(ctx, rv::sah_temp_bytes(n, &sah_bytes));
        temp_bytes = std::max(temp_bytes, sah_bytes);
    }
    const size_t node_cap = 2u * static_cast<size_t>(n) + 2u;  // 2 leaves - 1 nodes and the unused slot 1, leaves <= triangles
    if ((rc = grow(ctx, ctx->d_tris, ctx->cap_tris, n_tris, sizeof(rvpt_triangle)))) return rc;
    if ((rc = grow(ctx, ctx->d_prep, ctx->cap_prep, n_tris, sizeof(rvpt_triangle)))) return rc;
    if ((rc = grow(ctx, ctx->d_mat_index, ctx->cap_mat_index, n_tris, sizeof(uint32_t)))) return rc;
    if ((rc = grow(ctx, ctx->d_unit_n, ctx->cap_unit_n, n_tris, sizeof(float4)))) return rc;
    if ((rc = grow(ctx, ctx->d_mats, ctx->cap_mats, n_mats, sizeof(rvpt_material)))) return rc;
    if ((rc = grow(ctx, ctx->d_perm, ctx->cap_perm, n_tris, sizeof(uint32_t)))) return rc;
    if ((rc = grow(ctx, ctx->d_nodes, ctx->cap_nodes, node_cap, sizeof(rvpt_bvh_node)))) return rc;
    if ((rc = grow(ctx, ctx->d_build, ctx->cap_build, scratch_bytes, 1))) return rc;
    if ((rc = grow(ctx, ctx->d_build_temp, ctx->cap_build_temp, temp_bytes, 1))) return rc;
    unsigned char *const base = ctx->d_build;
    uint64_t *const keys = reinterpret_cast<uint64_t *>(base), *const sorted = reinterpret_cast<uint64_t *>(base + 8u * static_cast<size_t>(n));
    uint2 *ranges = reinterpret_cast<uint2 *>(base), *ranges_next = reinterpret_cast<uint2 *>(base + 16u * static_cast<size_t>(n));
    uint32_t *flags = reinterpret_cast<uint32_t *>(base + 24u * static_cast<size_t>(n)), *flags_next = reinterpret_cast<uint32_t *>(base + 24u * static_cast<size_t>(n) + words);
    uint32_t *const offs = reinterpret_cast<uint32_t *>(base + 24u * static_cast<size_t>(n) + 2u * words);
    ctx->have_scene = false;  // from here on the stored scene is being replaced: an error below leaves none
    ctx->have_sparse_maps = ctx->have_inv_perm = ctx->have_surface_inv = false;  // ... and with it the topology and the permutation the sparse update's maps were made for
    if (n_mats) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mats, mats, n_mats * sizeof(rvpt_material), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(rv::prepare_materials, dim3((static_cast<uint32_t>(n_mats) + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_mats, static_cast<uint32_t>(n_mats));
        HIP_TRY(ctx, hipGetLastError());
    }
    const float4 *src = reinterpret_cast<const float4 *>(tris);
    if (!device_source) {  // a host array is staged in d_prep, which prepare_triangles rewrites at the end
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_prep, tris, n_tris * sizeof(rvpt_triangle), hipMemcpyHostToDevice, ctx->stream));
        src = ctx->d_prep;
    }
    std::vector<std::pair<uint32_t, uint32_t>> levels;
    const char *fell_back = nullptr;
    if (sah) {  // the SAH tree in place of stages 1 - 4 (rvpt_build.h: THE SAH TREE): one level = decide + emit, three words read, partition
        uint32_t height_bound = 30u + 1u;
        while (height_bound - 31u < 32u && (1ull << (height_bound - 31u)) < n) height_bound += 1u;  // 30 + ceil(log2 n) + 1
        height_bound = std::min(height_bound, rv::kBvhStackDepth);
        HIP_TRY(ctx, rv::sah_begin(ctx->stream, src, n, base, ctx->d_build_counters, ctx->d_nodes));
        uint32_t parity = 0, median_before = 0, large_seen = 0, large_base = 0, n_large = n > rv::kSahLargeNode ? 1u : 0u;  // (the root holds slot 0, as the first slot handed out will)
        for (uint32_t begin = 0, count = 1, next_begin = 2;;) {
            if (levels.size() >= height_bound)
                return fail(ctx, RVPT_HIP_ERR_INVALID, "device BVH build: the SAH tree is higher than the %u levels its definition allows for %u triangles", height_bound, n);
            const uint32_t depth = static_cast<uint32_t>(levels.size());
            levels.emplace_back(begin, begin + count);
            HIP_TRY(ctx, rv::sah_decide_level(ctx->stream, ctx->d_build_temp, temp_bytes, base, n, parity, depth, begin, count, next_begin, large_base, n_large, ctx->d_nodes,
                                              static_cast<uint32_t>(node_cap), ctx->d_build_counters));
            HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_build_counters + rv::kSahSplits, 3u * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            const uint32_t splits = h[0], median_total = h[1], large_total = h[2];
            if (splits == 0) break;
            if (splits > count || static_cast<size_t>(next_begin) + 2u * splits > node_cap || 2u * static_cast<uint64_t>(splits) > n)
                return fail(ctx, RVPT_HIP_ERR_HIP, "device BVH build: a level of %u pairs does not fit the node buffer", splits);
            HIP_TRY(ctx, rv::sah_partition_level(ctx->stream, ctx->d_build_temp, temp_bytes, base, n, parity, count, median_total - median_before));
            median_before = median_total;
            large_base = large_seen, n_large = large_total - large_seen, large_seen = large_total;
            begin = next_begin, count = 2u * splits, next_begin = begin + count;
            parity ^= 1u;
        }
        HIP_TRY(ctx, rv::sah_gather(ctx->stream, src, base, n, parity, ctx->d_tris, ctx->d_perm));
    } else {
        // stages 1-3: keys, sort, gather
        HIP_TRY(ctx, rv::build_keys(ctx->stream, src, n, ctx->d_build_counters, keys));
        HIP_TRY(ctx, rv::build_sort_keys(ctx->stream, ctx->d_build_temp, temp_bytes, keys, sorted, n));
        HIP_TRY(ctx, rv::build_gather(ctx->stream, src, sorted, n, ctx->d_tris, ctx->d_perm));
    }
    // stage 4: the topology, level by level, straight into the device layout (root at 0, slot 1 unused, sibling pairs on even indices, upper levels first)
    if (ploc) {  // the PLOC tree in place of stage 4 (rvpt_build.h); the sorted keys stay as they are for the fallback
        unsigned char *const scratch = base + lbvh_bytes;
        uint32_t m = n, parity = 0, iterations = 0;
        HIP_TRY(ctx, rv::ploc_begin(ctx->stream, reinterpret_cast<const float4 *>(ctx->d_tris), n, scratch));
        while (m > rv::kPlocTailClusters && iterations < rv::kPlocMaxIterations) {
            HIP_TRY(ctx, rv::ploc_iteration(ctx->stream, ctx->d_build_temp, temp_bytes, scratch, n, m, parity, flags, offs));
            uint32_t left = 0;
            HIP_TRY(ctx, read_word(left, offs + m));
            if (left == 0 || left >= m) return fail(ctx, RVPT_HIP_ERR_HIP, "device BVH build: a PLOC iteration left %u of %u clusters", left, m);
            m = left, parity ^= 1u, iterations += 1u;
        }
        uint32_t root_and_iterations[2] = {0u, 0xFFFFFFFFu};
        if (m <= rv::kPlocTailClusters) {
            HIP_TRY(ctx, rv::ploc_finish(ctx->stream, scratch, n, m, parity, iterations, ctx->d_build_counters));
            HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_build_counters + rv::kPlocRoot, 2u * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            root_and_iterations[0] = h[0], root_and_iterations[1] = h[1];
        }
        if (root_and_iterations[1] == 0xFFFFFFFFu) {
            fell_back = "it was not finished within the iterations allowed";
        } else {  // the layout: the level loop of stage 4 over the provisional nodes (the dead unsorted keys' region holds the two level arrays)
            uint32_t *cur = reinterpret_cast<uint32_t *>(base), *cur_next = cur + n;
            uint32_t *fl = flags, *fl_next = flags_next;
            HIP_TRY(ctx, rv::ploc_layout_root(ctx->stream, ctx->d_build_counters, n, cur, fl, ctx->d_nodes));
            for (uint32_t begin = 0, count = 1, next_begin = 2;;) {
                if (levels.size() >= rv::kPlocMaxHeight) {
                    fell_back = "it is higher than the levels allowed";
                    levels.clear();
                    break;
                }
                levels.emplace_back(begin, begin + count);
                HIP_TRY(ctx, rv::ploc_layout_level(ctx->stream, ctx->d_build_temp, temp_bytes, scratch, n, cur, fl, offs, begin, count, next_begin, cur_next, fl_next, ctx->d_nodes,
                                                   static_cast<uint32_t>(node_cap)));
                uint32_t inner = 0;
                HIP_TRY(ctx, read_word(inner, offs + count));
                if (inner == 0) break;
                if (static_cast<size_t>(next_begin) + 2u * inner > node_cap) return fail(ctx, RVPT_HIP_ERR_HIP, "device BVH build: a level of %u pairs does not fit the node buffer", inner);
                begin = next_begin, count = 2u * inner, next_begin = begin + count;
                std::swap(cur, cur_next);
                std::swap(fl, fl_next);
            }
            if (!fell_back && levels.back().second != (n == 1u ? 1u : 2u * n))
                return fail(ctx, RVPT_HIP_ERR_HIP, "device BVH build: the PLOC tree of %u triangles came out with %u node slots", n, levels.back().second);
        }
    }
    const bool lbvh_tree = levels.empty();
    if (lbvh_tree) HIP_TRY(ctx, rv::build_root(ctx->stream, n, ranges, flags, ctx->d_nodes));
    for (uint32_t begin = 0, count = 1, next_begin = 2; lbvh_tree;) {
        // rvpt_build.h: at most 30 + ceil(log2 n) + 1 <= 61 levels for n <= 2^30 triangles; counted, not clamped
        if (levels.size() >= rv::kBvhStackDepth)
            return fail(ctx, RVPT_HIP_ERR_INVALID, "device BVH build: the tree is higher than the %u levels the traversal stack can walk", rv::kBvhStackDepth);
        levels.emplace_back(begin, begin + count);
        HIP_TRY(ctx, rv::build_level(ctx->stream, ctx->d_build_temp, temp_bytes, sorted, ranges, flags, offs, begin, count, next_begin, ranges_next, flags_next, ctx->d_nodes,
                                     static_cast<uint32_t>(node_cap), ctx->d_build_counters));
        uint32_t inner = 0;
        HIP_TRY(ctx, read_word(inner, offs + count));
        if (inner == 0) break;
        if (static_cast<size_t>(next_begin) + 2u * inner > node_cap) return fail(ctx, RVPT_HIP_ERR_HIP, "device BVH build: a level of %u pairs does not fit the node buffer", inner);
        begin = next_begin, count = 2u * inner, next_begin = begin + count;
        std::swap(ranges, ranges_next);
        std::swap(flags, flags_next);
    }
    const size_t n_device_nodes = std::max<size_t>(2, levels.back().second);
    // stage 5: boxes, deepest level first
    for (size_t l = levels.size(); l-- > 0;) {
        const auto [begin, end] = levels[l];
        hipLaunchKernelGGL(rv::refit_level, dim3((end - begin + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_nodes, begin, end, static_cast<uint32_t>(n_device_nodes), ctx->d_tris, n);
    }
    HIP_TRY(ctx, hipGetLastError());
    // stage 6: can a node's (first, count) pair ride in one stack word?  (the rule of the full upload)
    uint32_t max_count = 0, head_shift = 0;
    if (lbvh_tree || sah) HIP_TRY(ctx, read_word(max_count, ctx->d_build_counters + rv::kBuildMaxLeaf));
    else max_count = 1;  // PLOC leaves hold one triangle
    {
        uint32_t shift = 1;
        while (shift < 31 && (1ull << shift) <= std::max(n_device_nodes, n_tris)) shift += 1;
        if (static_cast<uint64_t>(max_count) < (1ull << (32 - shift))) head_shift = shift;
    }
    // stage 7: the 4-wide form (bvh_wide.cpp: regroup as a level loop); no wide form for a single-leaf tree, heads that do not pack, need > 4096, kWideMaxNodes
    size_t n_wide_kept = 0;
    uint32_t wide_need_kept = 0;
    const size_t n_inner = (n_device_nodes - 2u) / 2u;
    // (the laboratory's caller-layout knob does not apply: there is no caller's layout — the tree is born breadth first, with its level table)
    const uint64_t wide_limit = std::min<uint64_t>(rv::kWideMaxNodes, 1ull << head_shift);  // a wide index must address 128-byte nodes in 32 bits and fit below a head's count bits
    if (levels.size() > 1 && head_shift != 0) {
        if ((rc = grow(ctx, ctx->d_wide_map, ctx->cap_wide_map, n_inner * 4u, sizeof(uint32_t)))) return rc;
        uint32_t *const heads = reinterpret_cast<uint32_t *>(base);  // 16 bytes per wide node, <= 16 (n - 1)
        uint32_t *bin = reinterpret_cast<uint32_t *>(base + 16u * static_cast<size_t>(n)), *bin_next = bin + n;
        uint32_t *const cnt = flags, *const need = flags_next;
        std::vector<std::pair<uint32_t, uint32_t>> wide_levels;  // (first wide index, count)
        HIP_TRY(ctx, rv::build_wide_root(ctx->stream, bin));
        uint32_t wbase = 0, count = 1;
        for (;;) {
            if (wide_levels.size() >= levels.size()) return fail(ctx, RVPT_HIP_ERR_HIP, "device BVH build: the wide form has more levels than the binary tree");
            wide_levels.emplace_back(wbase, count);
            HIP_TRY(ctx, rv::build_wide_level(ctx->stream, ctx->d_build_temp, temp_bytes, ctx->d_nodes, static_cast<uint32_t>(n_device_nodes), bin, wbase, count, head_shift, cnt, offs,
                                              ctx->d_wide_map, heads, static_cast<uint32_t>(n_inner), bin_next));
            uint32_t next = 0;
            HIP_TRY(ctx, read_word(next, offs + count));
            if (next == 0) break;
            // (wide_pick / wide_emit write nothing beyond n_inner rows and leave a level partly written when it would not fit: this check is what makes that safe)
            if (static_cast<size_t>(wbase) + count + next > n_inner) return fail(ctx, RVPT_HIP_ERR_HIP, "device BVH build: more wide nodes than inner nodes");
            wbase += count, count = next;
            if (static_cast<uint64_t>(wbase) + count >= wide_limit) break;  // no wide form for this tree: the levels below need not be made
            std::swap(bin, bin_next);
        }
        const size_t n_wide = static_cast<size_t>(wbase) + count;
        if (n_wide < wide_limit) {
            if ((rc = grow(ctx, ctx->d_wide, ctx->cap_wide, n_wide * 8, sizeof(float4)))) return rc;
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_wide, 0, n_wide * 128u, ctx->stream));  // unused slots and padding are zero, as build_wide_nodes leaves them
            HIP_TRY(ctx, rv::build_wide_heads(ctx->stream, heads, static_cast<uint32_t>(n_wide), reinterpret_cast<float *>(ctx->d_wide)));
            const uint32_t n_slots = static_cast<uint32_t>(n_wide * 4);
            hipLaunchKernelGGL(rv::refit_wide_gather, dim3((n_slots + 255u) / 256u), dim3(256), 0, ctx->stream, reinterpret_cast<float *>(ctx->d_wide), ctx->d_wide_map, n_slots, ctx->d_nodes,
                               static_cast<uint32_t>(n_device_nodes));
            HIP_TRY(ctx, hipGetLastError());
            for (size_t l = wide_levels.size(); l-- > 0;)  // the same bottom-up maximum as need[] in bvh_wide.cpp
                HIP_TRY(ctx, rv::build_wide_need(ctx->stream, reinterpret_cast<const float *>(ctx->d_wide), wide_levels[l].first, wide_levels[l].second, static_cast<uint32_t>(n_wide), head_shift, need));
            uint32_t root_need = 0;
            HIP_TRY(ctx, read_word(root_need, need));
            root_need = std::max(1u, root_need);
            if (root_need <= 4096u) n_wide_kept = n_wide, wide_need_kept = root_need;
        }
    }
    // stage 8: what the full upload derives from d_tris
    if ((rc = launch_prepare_triangles(ctx, n_tris))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // caller may free its arrays on return
    ctx->n_tris = n_tris;
    ctx->n_mats = n_mats;
    ctx->n_nodes = n_device_nodes;
    ctx->bvh_height = static_cast<uint32_t>(levels.size());
    ctx->refit_levels = std::move(levels);
    ctx->bvh_head_shift = head_shift;
    ctx->n_wide = n_wide_kept;
    ctx->wide_stack_levels = wide_need_kept;
    ctx->have_perm = true;
    if ((rc = derive_bounce_state(ctx, true, nullptr, n_tris))) return rc;
    if ((rc = device_tree_cost(ctx, &ctx->base_cost, &ctx->have_cost))) return rc;  // the base cost of the guarded update
    ctx->built_by = sah ? rvpt_hip_ctx::kBuiltSah : ploc ? rvpt_hip_ctx::kBuiltPloc : rvpt_hip_ctx::kBuiltLbvh;  // (a PLOC build that fell back is rebuilt as PLOC, by the same rule)
    if (mats != ctx->host_mats.data() || n_mats != ctx->host_mats.size()) ctx->host_mats.assign(mats, mats + n_mats);  // (a guarded rebuild passes the stored array itself)
    ctx->scene_gen += 1;  // the slots' screen rectangles belong to the old scene
    ctx->have_scene = true;
    if (ploc) {  // which tree this was: the one fact a PLOC build reports beside its return code
        if (fell_back) fail(ctx, RVPT_HIP_OK, "device BVH build: the PLOC tree was dropped (%s), the scene holds the LBVH tree", fell_back);
        else ctx->err.clear();
    }
    if (sah) ctx->err.clear();
    return RVPT_HIP_OK;
}

// the sparse update's list, checked on the host: the smallest position whose index is out of range, else the smallest index that occurs twice; the span of the indices
static int sparse_validate_host(rvpt_hip_ctx *ctx, const uint32_t *indices, size_t k, size_t n_tris, uint32_t *lo_out, uint32_t *hi_out)
{
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (size_t j = 0; j < k; ++j) {
        if (indices[j] >= n_tris) return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: indices[%zu] = %u is outside the %zu stored triangles", j, indices[j], n_tris);
        lo = std::min(lo, indices[j]), hi = std::max(hi, indices[j]);
    }
    std::vector<uint32_t> sorted(indices, indices + k);
    std::sort(sorted.begin(), sorted.end());
    for (size_t j = 1; j < k; ++j)
        if (sorted[j] == sorted[j - 1]) return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: index %u occurs more than once in the list", sorted[j]);
    *lo_out = lo, *hi_out = hi;
    return RVPT_HIP_OK;
}

// What the sparse update and the pose update share (BVH contexts with a level table).
// The permutation's inverse: after a build form the caller's indices are not positions.  It reads and writes nothing a frame in flight uses.
static int ensure_inverse_permutation(rvpt_hip_ctx *ctx)
{
    if (!ctx->have_perm || ctx->have_inv_perm) return RVPT_HIP_OK;
    const size_t n_tris = ctx->n_tris;
    const uint32_t n = static_cast<uint32_t>(n_tris);
    if (int rc = grow(ctx, ctx->d_inv_perm, ctx->cap_inv_perm, n_tris, sizeof(uint32_t))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_inv_perm, 0xFF, n_tris * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(rv::sparse_invert_permutation, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_perm, n, ctx->d_inv_perm);
    HIP_TRY(ctx, hipGetLastError());
    ctx->have_inv_perm = true;
    return RVPT_HIP_OK;
}

// The maps of the stored topology, made on the first sparse or pose update after any full upload, build or rebuild.  n_nodes: the end of the last level.
static int ensure_sparse_maps(rvpt_hip_ctx *ctx, uint32_t n_nodes)
{
    if (ctx->have_sparse_maps) return RVPT_HIP_OK;
    int rc;
    const size_t n_tris = ctx->n_tris;
    if ((rc = grow(ctx, ctx->d_sparse_parent, ctx->cap_sparse_parent, n_nodes, sizeof(uint32_t)))) return rc;
    if ((rc = grow(ctx, ctx->d_sparse_dirty, ctx->cap_sparse_dirty, n_nodes, sizeof(uint32_t)))) return rc;
    if ((rc = grow(ctx, ctx->d_sparse_leaf_of, ctx->cap_sparse_leaf_of, n_tris, sizeof(uint32_t)))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_sparse_parent, 0xFF, n_nodes * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_sparse_dirty, 0, n_nodes * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_sparse_leaf_of, 0xFF, n_tris * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(rv::sparse_topology, dim3((n_nodes + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_nodes, n_nodes, static_cast<uint32_t>(n_tris), ctx->d_sparse_parent,
                       ctx->d_sparse_leaf_of);
    HIP_TRY(ctx, hipGetLastError());
    return RVPT_HIP_OK;
}

// The tail of both forms, behind the launch that wrote the rows of d_tris and flagged their paths (have_sparse_maps is false while flags may be set):
// prepare_triangles as it is over the rows [span_lo, span_hi] — records, material index slots and unit normals —, the flagged nodes refitted level by level,
// deepest first, the wide form's copies gathered again, and the stream waited for: the caller may free its arrays on return.
static int refit_flagged_paths(rvpt_hip_ctx *ctx, uint32_t n_nodes, uint32_t span_lo, uint32_t span_hi)
{
    const uint32_t n = static_cast<uint32_t>(ctx->n_tris);
    {
        const uint32_t rows = span_hi - span_lo + 1u;
        hipLaunchKernelGGL(rv::prepare_triangles, dim3((rows + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_tris + 4u * static_cast<size_t>(span_lo), rows,
                           ctx->d_prep + 4u * static_cast<size_t>(span_lo), ctx->d_mat_index + span_lo, ctx->d_unit_n + span_lo);
        HIP_TRY(ctx, hipGetLastError());
    }
    for (size_t l = ctx->refit_levels.size(); l-- > 0;) {
        const auto [begin, end] = ctx->refit_levels[l];
        hipLaunchKernelGGL(rv::refit_level_dirty, dim3((end - begin + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_nodes, begin, end, n_nodes, ctx->d_tris, n, ctx->d_sparse_dirty);
    }
    if (ctx->n_wide) {
        const uint32_t n_slots = static_cast<uint32_t>(ctx->n_wide * 4);
        hipLaunchKernelGGL(rv::refit_wide_gather, dim3((n_slots + 255u) / 256u), dim3(256), 0, ctx->stream, reinterpret_cast<float *>(ctx->d_wide), ctx->d_wide_map, n_slots, ctx->d_nodes,
                           static_cast<uint32_t>(ctx->n_nodes));
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_sparse_maps = true;
    ctx->scene_gen += 1;  // the slots' screen rectangles and sky lists belong to the old geometry
    return RVPT_HIP_OK;
}

// The SPARSE UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): `indices` names k stored triangles, tris[j] replaces the vertices of triangle indices[j].
// Everything is validated before anything stored is touched — a host list on the host, a device list by two kernels and one read of four words, with the same
// answers.  BVH contexts: the rows are scattered into d_tris, the paths from their leaves to the root are flagged, prepare_triangles runs over the span of rows
// the list touches, the flagged nodes are refitted level by level (deepest first) and the wide form's copies of the boxes are gathered again; every other box
// stays as it is.  Brute-force contexts derive their scale, table and boxes from the whole vertex set on the host: the stored records are read back, patched,
// and go through the plain update form.
static int update_geometry_sparse(rvpt_hip_ctx *ctx, const uint32_t *indices, const rvpt_triangle *tris, size_t k, const rvpt_material *mats, size_t n_mats)
{
    if (!ctx->have_scene)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update before any full upload_scene on this context: there is no scene to update");
    if (k == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update without triangles");
    const size_t n_tris = ctx->n_tris;
    if (k > n_tris) return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update with %zu triangles, the uploaded scene has %zu", k, n_tris);
    if (!indices) return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update without indices: `nodes` points at one uint32_t per triangle passed");
    if (mats || n_mats) return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update takes no materials: it keeps the stored ones");
    if (reinterpret_cast<uintptr_t>(indices) % 4u) return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: the indices at %p are not 4-byte aligned", static_cast<const void *>(indices));
    const bool bvh = is_bvh(ctx, n_tris);
    if (bvh && ctx->refit_levels.empty())  // (the laboratory's knob only, as in the plain form)
#if RVPT_HIP_LAB
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the breadth-first device layout of the tree: RVPT_HIP_BVH_CALLER_LAYOUT keeps the caller's, which has no level ranges");
#else
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the level ranges of the tree's device layout, which this context does not hold");
#endif
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool device_tris = is_device_pointer(tris), device_indices = is_device_pointer(indices);
    if (!bvh && (device_tris || device_indices))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "geometry update of a brute-force context from a device pointer: its scene scale and leaf boxes are computed on the host, pass a host array");
    if (device_tris != device_indices)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: the indices are %s memory and the triangles %s memory: both on the host or both on the context's GPU",
                    device_indices ? "device" : "host", device_tris ? "device" : "host");
    if (device_tris) {
        const void *const both[2] = {indices, tris};
        for (int i = 0; i < 2; ++i) {
            hipPointerAttribute_t attr{};
            HIP_TRY(ctx, hipPointerGetAttributes(&attr, both[i]));
            if (attr.device != ctx->device)
                return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: the %s are device memory of GPU %d, the context lives on GPU %d", i ? "triangles" : "indices", attr.device, ctx->device);
        }
        if (reinterpret_cast<uintptr_t>(tris) % 16u)
            return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: triangles in device memory at %p need 16-byte alignment", static_cast<const void *>(tris));
    }
    const uint32_t n = static_cast<uint32_t>(n_tris), kk = static_cast<uint32_t>(k);
    uint32_t span_lo = 0, span_hi = 0;

    if (!bvh) {  // host arrays: validate, read the stored records back, patch, the plain form
        if (int rc0 = sparse_validate_host(ctx, indices, k, n_tris, &span_lo, &span_hi)) return rc0;
        if (int rc0 = sync_all(ctx)) return rc0;
        std::vector<rvpt_triangle> patched(n_tris);
        HIP_TRY(ctx, hipMemcpy(patched.data(), ctx->d_tris, n_tris * sizeof(rvpt_triangle), hipMemcpyDeviceToHost));
        for (size_t j = 0; j < k; ++j) std::memcpy(&patched[indices[j]], &tris[j], offsetof(rvpt_triangle, mat_id));
        return update_geometry(ctx, patched.data(), n_tris);
    }

    int rc;
    const uint32_t n_nodes = static_cast<uint32_t>(std::min<size_t>(ctx->n_nodes, ctx->refit_levels.back().second));
    const uint32_t *d_indices = indices;
    const float4 *d_src = reinterpret_cast<const float4 *>(tris);
    if (!device_tris && (rc = sparse_validate_host(ctx, indices, k, n_tris, &span_lo, &span_hi))) return rc;
    // the permutation's inverse is needed by the device validation's span, so made in front of it; a device list that is then refused leaves the flag as it
    // found it: a refusal changes nothing the context holds, the inverse a later update would make included
    const bool had_inv_perm = ctx->have_inv_perm;
    if ((rc = ensure_inverse_permutation(ctx))) return rc;
    const uint32_t *const inv_perm = ctx->have_perm ? ctx->d_inv_perm : nullptr;
    if (!device_tris) {  // a validated host list is staged: the indices behind the records
        if (inv_perm) span_lo = 0, span_hi = n - 1u;  // (the positions are known on the device alone: the whole buffer)
        if ((rc = grow(ctx, ctx->d_sparse_stage, ctx->cap_sparse_stage, k * (sizeof(rvpt_triangle) + sizeof(uint32_t)), 1))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sparse_stage, tris, k * sizeof(rvpt_triangle), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sparse_stage + k * sizeof(rvpt_triangle), indices, k * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        d_src = reinterpret_cast<const float4 *>(ctx->d_sparse_stage);
        d_indices = reinterpret_cast<const uint32_t *>(ctx->d_sparse_stage + k * sizeof(rvpt_triangle));
    } else {  // a device list: two kernels and one read of four words
        size_t cap_words = ctx->d_sparse_words ? rv::kSparseWords : 0;
        if ((rc = grow(ctx, ctx->d_sparse_words, cap_words, rv::kSparseWords, sizeof(uint32_t)))) return rc;
        if (!ctx->h_sparse_words) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_sparse_words), rv::kSparseWords * sizeof(uint32_t)));
        if ((rc = grow(ctx, ctx->d_sparse_claim, ctx->cap_sparse_claim, n_tris, sizeof(uint32_t)))) return rc;
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_sparse_claim, 0xFF, n_tris * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_sparse_words, 0xFF, 3u * sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_sparse_words + rv::kSparseSpanHi, 0, sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(rv::sparse_claim, dim3((kk + 255u) / 256u), dim3(256), 0, ctx->stream, d_indices, kk, n, inv_perm, ctx->d_sparse_claim, ctx->d_sparse_words);
        hipLaunchKernelGGL(rv::sparse_duplicates, dim3((kk + 255u) / 256u), dim3(256), 0, ctx->stream, d_indices, kk, n, ctx->d_sparse_claim, ctx->d_sparse_words);
        HIP_TRY(ctx, hipGetLastError());
        uint32_t *const h = ctx->h_sparse_words;
        HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_sparse_words, rv::kSparseWords * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (h[rv::kSparseBadPosition] != 0xFFFFFFFFu) {
            const size_t j = h[rv::kSparseBadPosition];
            uint32_t value = 0;
            if (j < k) HIP_TRY(ctx, hipMemcpy(&value, indices + j, sizeof value, hipMemcpyDeviceToHost));
            ctx->have_inv_perm = had_inv_perm;
            return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: indices[%zu] = %u is outside the %zu stored triangles", j, value, n_tris);
        }
        if (h[rv::kSparseDuplicate] != 0xFFFFFFFFu) {
            ctx->have_inv_perm = had_inv_perm;
            return fail(ctx, RVPT_HIP_ERR_INVALID, "sparse update: index %u occurs more than once in the list", h[rv::kSparseDuplicate]);
        }
        span_lo = h[rv::kSparseSpanLo], span_hi = h[rv::kSparseSpanHi];
        if (span_lo > span_hi || span_hi >= n) span_lo = 0, span_hi = n - 1u;
    }
    if ((rc = ensure_sparse_maps(ctx, n_nodes))) return rc;
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight finish on the old geometry
    ctx->have_sparse_maps = false;  // (until the flags are known to be all zero again: after an error below the next update starts from fresh maps)
    hipLaunchKernelGGL(rv::sparse_scatter, dim3((kk + 255u) / 256u), dim3(256), 0, ctx->stream, d_src, d_indices, kk, n, inv_perm, ctx->d_tris, ctx->d_sparse_leaf_of, ctx->d_sparse_parent,
                       n_nodes, ctx->d_sparse_dirty);
    HIP_TRY(ctx, hipGetLastError());
    return refit_flagged_paths(ctx, n_nodes, span_lo, span_hi);
}

// the pose update's list, checked on the host before anything stored is touched: per record, in list order, a count of 0, a non-zero reserved word, a range
// that leaves the stored scene (the first position that offends in any of these ways is named); then two ranges that share a triangle — the ranges are sorted
// by `first`, as sparse_validate_host sorts indices, and the message names the smallest pair of list positions (i, j), i < j, whose ranges meet.  total_out: the
// triangles listed; lo_out / hi_out: the span of their indices.
static int pose_validate_host(rvpt_hip_ctx *ctx, const rvpt_part_move *moves, size_t k, size_t n_tris, uint32_t *total_out, uint32_t *lo_out, uint32_t *hi_out)
{
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (size_t p = 0; p < k; ++p) {
        const rvpt_part_move &m = moves[p];
        if (m.count == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update: moves[%zu] has a count of 0: a part holds at least one triangle", p);
        if (m.reserved[0] != 0 || m.reserved[1] != 0)
            return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update: moves[%zu] has the reserved words %u, %u: they must be 0", p, m.reserved[0], m.reserved[1]);
        if (m.first >= n_tris || m.count > n_tris - m.first)  // (first + count > n_tris, without the sum)
            return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update: moves[%zu] = [%u, %u + %u) is outside the %zu stored triangles", p, m.first, m.first, m.count, n_tris);
        lo = std::min(lo, m.first), hi = std::max(hi, m.first + (m.count - 1u));
    }
    std::vector<uint32_t> order(k);
    for (size_t p = 0; p < k; ++p) order[p] = static_cast<uint32_t>(p);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return moves[a].first != moves[b].first ? moves[a].first < moves[b].first : a < b; });
    // a range meets another iff it meets one of its neighbours in the sorted order, the furthest-reaching range in front of it taken for the predecessor
    size_t smallest = k;
    uint64_t reach = 0;  // the largest end of the ranges in front of slot s
    for (size_t s = 0; s < k; ++s) {
        const rvpt_part_move &m = moves[order[s]];
        const uint64_t end = static_cast<uint64_t>(m.first) + m.count;
        const bool meets = (s > 0 && reach > m.first) || (s + 1 < k && moves[order[s + 1]].first < end);
        if (meets) smallest = std::min<size_t>(smallest, order[s]);
        reach = std::max(reach, end);
    }
    if (smallest < k) {
        const rvpt_part_move &a = moves[smallest];
        for (size_t q = 0; q < k; ++q) {  // (every range that meets moves[smallest] lies behind it in the list: it is the smallest position that meets any)
            const rvpt_part_move &b = moves[q];
            if (q == smallest || static_cast<uint64_t>(b.first) >= static_cast<uint64_t>(a.first) + a.count || static_cast<uint64_t>(a.first) >= static_cast<uint64_t>(b.first) + b.count) continue;
            return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update: moves[%zu] = [%u, %u + %u) and moves[%zu] = [%u, %u + %u) share triangle %u: a triangle belongs to one part", smallest,
                        a.first, a.first, a.count, q, b.first, b.first, b.count, std::max(a.first, b.first));
        }
    }
    *total_out = 0;
    for (size_t p = 0; p < k; ++p) *total_out += moves[p].count;  // (disjoint ranges inside the scene: at most n_tris)
    *lo_out = lo, *hi_out = hi;
    return RVPT_HIP_OK;
}

// one vertex through one 3x4 matrix, the host form of rv::pose_vertex: three products and three sums per component, each rounded to binary32 on its own, in the
// order ((m0 x + m1 y) + m2 z) + m3.  This file is compiled with -ffp-contract=off (rvpt_amd/build.py), so the expressions below are not fused.
static void pose_vertex_host(const float m[12], const float p[3], float out[3])
{
    for (int i = 0; i < 3; ++i) {
        const float a = m[4 * i] * p[0], b = m[4 * i + 1] * p[1], c = m[4 * i + 2] * p[2];
        const float ab = a + b;
        const float abc = ab + c;
        out[i] = abc + m[4 * i + 3];
    }
}

// The POSE UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): `moves` names k disjoint ranges of stored triangles and one 3x4 matrix per range.  Everything is
// validated on the host before anything stored is touched.  BVH contexts: the rest pose is snapshotted on the device if the context holds none for the stored
// scene, rv::pose_parts poses the listed rows of d_tris from it and flags their paths, and the sparse update's tail does the rest.  Brute-force contexts keep the
// rest pose on the host: the stored records are read back, the listed ranges are posed there, and the plain update form runs.
// (Two halves, so that the guarded pose form can put its own refusal between them: pose_validate touches nothing stored, pose_execute refuses nothing a
// caller's arguments decide.)
struct PoseList {
    uint32_t total = 0, span_lo = 0, span_hi = 0;  // the triangles listed, the span of their indices
    bool bvh = false;
};

static int pose_validate(rvpt_hip_ctx *ctx, const rvpt_part_move *moves, const rvpt_triangle *tris, size_t k, const rvpt_material *mats, size_t n_mats, PoseList *list)
{
    if (!ctx->have_scene) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update before any full upload_scene on this context: there is no scene to update");
    if (k == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update without parts");
    const size_t n_tris = ctx->n_tris;
    if (k > n_tris) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update with %zu parts, the uploaded scene has %zu triangles", k, n_tris);
    if (!moves) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update without a list: `nodes` points at one rvpt_part_move per part");
    if (reinterpret_cast<uintptr_t>(moves) % 4u) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update: the list at %p is not 4-byte aligned", static_cast<const void *>(moves));
    if (tris) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update takes no triangles: the library poses the ones it holds (`tris` must be NULL)");
    if (mats || n_mats) return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update takes no materials: it keeps the stored ones");
    const bool bvh = is_bvh(ctx, n_tris);
    if (bvh && ctx->refit_levels.empty())  // (the laboratory's knob only, as in the plain form)
#if RVPT_HIP_LAB
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the breadth-first device layout of the tree: RVPT_HIP_BVH_CALLER_LAYOUT keeps the caller's, which has no level ranges");
#else
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the level ranges of the tree's device layout, which this context does not hold");
#endif
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (is_device_pointer(moves))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "pose update: the list at %p is device memory: this form takes its list from the host (64 bytes per part)", static_cast<const void *>(moves));
    list->bvh = bvh;
    return pose_validate_host(ctx, moves, k, n_tris, &list->total, &list->span_lo, &list->span_hi);
}

static int pose_execute(rvpt_hip_ctx *ctx, const rvpt_part_move *moves, size_t k, const PoseList &list)
{
    const size_t n_tris = ctx->n_tris;
    const bool bvh = list.bvh;
    const uint32_t total = list.total;
    uint32_t span_lo = list.span_lo, span_hi = list.span_hi;
    const uint32_t n = static_cast<uint32_t>(n_tris), kk = static_cast<uint32_t>(k);

    if (!bvh) {  // the rest pose on the host, the posed records through the plain form
        if (int rc0 = sync_all(ctx)) return rc0;
        std::vector<rvpt_triangle> posed(n_tris);
        HIP_TRY(ctx, hipMemcpy(posed.data(), ctx->d_tris, n_tris * sizeof(rvpt_triangle), hipMemcpyDeviceToHost));
        if (!ctx->have_rest) {
            ctx->h_rest.resize(12 * n_tris);
            for (size_t t = 0; t < n_tris; ++t) std::memcpy(&ctx->h_rest[12 * t], &posed[t], offsetof(rvpt_triangle, mat_id));
            ctx->have_rest = true;
        }
        for (size_t p = 0; p < k; ++p)
            for (size_t t = moves[p].first; t < static_cast<size_t>(moves[p].first) + moves[p].count; ++t) {
                const float *r = &ctx->h_rest[12 * t];
                float *rows[3] = {posed[t].vert0, posed[t].vert1, posed[t].vert2};
                for (int v = 0; v < 3; ++v) {
                    pose_vertex_host(moves[p].m, r + 4 * v, rows[v]);
                    rows[v][3] = r[4 * v + 3];
                }
            }
        const int rc0 = update_geometry(ctx, posed.data(), n_tris);
        if (rc0 == RVPT_HIP_OK) ctx->err.clear();
        return rc0;
    }

    int rc;
    const uint32_t n_nodes = static_cast<uint32_t>(std::min<size_t>(ctx->n_nodes, ctx->refit_levels.back().second));
    if ((rc = ensure_inverse_permutation(ctx))) return rc;
    const uint32_t *const inv_perm = ctx->have_perm ? ctx->d_inv_perm : nullptr;
    if (inv_perm) span_lo = 0, span_hi = n - 1u;  // (the positions are known on the device alone: the whole buffer)
    // the list and the exclusive sums of its counts, staged where a sparse update stages its rows
    std::vector<uint32_t> prefix(k + 1);
    prefix[0] = 0;
    for (size_t p = 0; p < k; ++p) prefix[p + 1] = prefix[p] + moves[p].count;
    if ((rc = grow(ctx, ctx->d_sparse_stage, ctx->cap_sparse_stage, k * sizeof(rvpt_part_move) + (k + 1) * sizeof(uint32_t), 1))) return rc;
    if ((rc = ensure_sparse_maps(ctx, n_nodes))) return rc;
    if (!ctx->have_rest && (rc = grow(ctx, ctx->d_rest, ctx->cap_rest, 3 * n_tris, sizeof(float4)))) return rc;
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight finish on the old geometry
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sparse_stage, moves, k * sizeof(rvpt_part_move), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sparse_stage + k * sizeof(rvpt_part_move), prefix.data(), (k + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    if (!ctx->have_rest) {  // the snapshot: 48 of every 64 bytes of d_tris, device to device, in stored order
        HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_rest, offsetof(rvpt_triangle, mat_id), ctx->d_tris, sizeof(rvpt_triangle), offsetof(rvpt_triangle, mat_id), n_tris, hipMemcpyDeviceToDevice,
                                      ctx->stream));
        ctx->have_rest = true;
    }
    ctx->have_sparse_maps = false;  // (until the flags are known to be all zero again, as in the sparse update)
    hipLaunchKernelGGL(rv::pose_parts, dim3((total + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_rest, reinterpret_cast<const uint32_t *>(ctx->d_sparse_stage),
                       reinterpret_cast<const uint32_t *>(ctx->d_sparse_stage + k * sizeof(rvpt_part_move)), kk, total, n, inv_perm, ctx->d_tris, ctx->d_sparse_leaf_of, ctx->d_sparse_parent,
                       n_nodes, ctx->d_sparse_dirty);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = refit_flagged_paths(ctx, n_nodes, span_lo, span_hi))) {  // (prefix is read by the copy above until the stream has been waited for)
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    ctx->err.clear();
    return RVPT_HIP_OK;
}

static int update_geometry_pose(rvpt_hip_ctx *ctx, const rvpt_part_move *moves, const rvpt_triangle *tris, size_t k, const rvpt_material *mats, size_t n_mats)
{
    PoseList list;
    if (int rc = pose_validate(ctx, moves, tris, k, mats, n_mats, &list)) return rc;
    return pose_execute(ctx, moves, k, list);
}

// The rebuild tail of the guarded pose and the guarded skin update, behind their decision: the stored triangles and the rest pose into the caller's order by
// the old permutation, the build by the builder that made the stored tree, the rest pose back into stored order by the new permutation, and the report.
// `form`: "pose" or "skin", the word of the report.  d_skin is not touched: it is in the caller's order and is read through d_perm.
static int rebuild_keeping_rest(rvpt_hip_ctx *ctx, const char *form, double cost, double base, uint32_t permille)
{
    // the rebuild, as the guarded update's: d_tris (moved vertices beside the stored mat_id rows, leaf order) into d_carry in the caller's order, and beside it
    // the rest pose into d_rest_carry by the same permutation, before the build writes a new one
    const size_t n_tris = ctx->n_tris;
    const uint32_t n = static_cast<uint32_t>(n_tris);
    const int built_by = ctx->built_by;
    if (int rc = grow(ctx, ctx->d_carry, ctx->cap_carry, n_tris * 4u, sizeof(float4))) return rc;
    if (int rc = grow(ctx, ctx->d_rest_carry, ctx->cap_rest_carry, n_tris * 3u, sizeof(float4))) return rc;
    const uint32_t rest_blocks = static_cast<uint32_t>((3ull * n + 255u) / 256u);
    hipLaunchKernelGGL(rv::carry_back_triangles, dim3(static_cast<uint32_t>((4ull * n + 255u) / 256u)), dim3(256), 0, ctx->stream, ctx->d_tris, ctx->d_perm, n, ctx->d_carry);
    hipLaunchKernelGGL(rv::rest_to_caller_order, dim3(rest_blocks), dim3(256), 0, ctx->stream, ctx->d_rest, ctx->d_perm, n, ctx->d_rest_carry);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_rest = false;  // (d_rest is in the order of a permutation that is about to go: an error below leaves no rest pose)
    if (int rc = build_scene_on_device(ctx, reinterpret_cast<const rvpt_triangle *>(ctx->d_carry), n_tris, ctx->host_mats.data(), ctx->host_mats.size(), built_by == rvpt_hip_ctx::kBuiltPloc,
                                       built_by == rvpt_hip_ctx::kBuiltSah))
        return rc;  // the build form's rule: its message, and no scene after anything but a bad material index (which stored rows cannot hold)
    // (a PLOC build that fell back has left its sentence: the scene then holds the LBVH tree, and the report names it)
    const bool fell_back = built_by == rvpt_hip_ctx::kBuiltPloc && !ctx->err.empty();
    hipLaunchKernelGGL(rv::rest_to_stored_order, dim3(rest_blocks), dim3(256), 0, ctx->stream, ctx->d_rest_carry, ctx->d_perm, n, ctx->d_rest);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_rest = true;
    static const char *const kNames[] = {"", "lbvh", "ploc", "sah"};
    fail(ctx, RVPT_HIP_OK, "guarded %s update: cost %.17g, base cost %.17g, limit %u permille: rebuilt (%s), new base cost %.17g", form, cost, base, permille,
         kNames[fell_back ? rvpt_hip_ctx::kBuiltLbvh : built_by], ctx->base_cost);
    return RVPT_HIP_OK;
}

// The GUARDED POSE UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): the pose update, then the cost of the stored tree — the boxes off the listed paths as
// they were, loose ones included —, then, with a limit, once the cost has grown past limit x base cost, a rebuild by the builder that made the stored tree
// from the posed triangles carried back into the caller's order.  The rest pose goes with the rebuild: into the caller's order by the old permutation, back
// into stored order by the new one, so that the next pose update poses from the same rest pose as before.  permille: 0 (report only) or 1000 .. 65535, checked
// by the caller.  Brute-force contexts hold no tree: the plain pose form.
static int update_geometry_pose_guarded(rvpt_hip_ctx *ctx, const rvpt_part_move *moves, const rvpt_triangle *tris, size_t k, const rvpt_material *mats, size_t n_mats, uint32_t permille)
{
    // the pose form's own refusals come first, in its words and its order; then the one refusal of this form, before anything of the stored scene is touched
    PoseList list;
    if (int rc = pose_validate(ctx, moves, tris, k, mats, n_mats, &list)) return rc;
    if (!list.bvh) return pose_execute(ctx, moves, k, list);
    if (permille != 0 && ctx->built_by == rvpt_hip_ctx::kBuiltByCaller)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded pose update with a limit after an ordinary upload_scene: the tree is the caller's, the library has no builder to rebuild it by (report only, limit 0, is legal)");
    if (int rc = pose_execute(ctx, moves, k, list)) return rc;
    double cost = 0.0;
    bool have = false;
    if (int rc = device_tree_cost(ctx, &cost, &have)) return rc;
    const double base = ctx->base_cost;
    if (permille == 0 || !have || !ctx->have_cost || !ctx->have_perm || !(cost > static_cast<double>(permille) / 1000.0 * base)) {
        fail(ctx, RVPT_HIP_OK, "guarded pose update: cost %.17g, base cost %.17g, limit %u permille: refitted", cost, base, permille);
        return RVPT_HIP_OK;
    }
    return rebuild_keeping_rest(ctx, "pose", cost, base, permille);
}

// is `p` device memory, and of which GPU (-1: host memory)?
static int device_of_pointer(const void *p)
{
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return attr.type == hipMemoryTypeDevice ? attr.device : -1;
}

static void drop_skin(rvpt_hip_ctx *ctx)
{
    ctx->have_skin = false;
    ctx->skin_bones = 0;
}

// The BIND of rvpt_hip_upload_scene (include/rvpt_hip.h): three rvpt_vertex_skin records per stored triangle, in the order the plain update form takes, copied
// into d_skin (BVH contexts) or h_skin (brute-force contexts) once every refusal is behind.  A host list is checked here, a device list by rv::skin_check and
// one read of its four words.  Moves nothing, keeps the rest pose, leaves scene_gen alone.
static int bind_skin(rvpt_hip_ctx *ctx, const rvpt_vertex_skin *skin, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t n_mats)
{
    if (!ctx->have_scene) return fail(ctx, RVPT_HIP_ERR_INVALID, "bind before any full upload_scene on this context: there is no scene to bind weights to");
    if (n_tris != ctx->n_tris) return fail(ctx, RVPT_HIP_ERR_INVALID, "bind for %zu triangles, the uploaded scene has %zu: three records per stored triangle", n_tris, ctx->n_tris);
    if (!skin) return fail(ctx, RVPT_HIP_ERR_INVALID, "bind without a list: `nodes` points at three rvpt_vertex_skin records per triangle");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int dev = device_of_pointer(skin);
    if (reinterpret_cast<uintptr_t>(skin) % (dev >= 0 ? 16u : 4u))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "bind: the list at %p is not %u-byte aligned", static_cast<const void *>(skin), dev >= 0 ? 16u : 4u);
    if (tris) return fail(ctx, RVPT_HIP_ERR_INVALID, "bind takes no triangles: the weights belong to the stored ones (`tris` must be NULL)");
    if (mats || n_mats) return fail(ctx, RVPT_HIP_ERR_INVALID, "bind takes no materials: it keeps the stored ones");
    const bool bvh = is_bvh(ctx, n_tris);
    if (dev >= 0 && dev != ctx->device) return fail(ctx, RVPT_HIP_ERR_INVALID, "bind: the list is device memory of GPU %d, the context lives on GPU %d", dev, ctx->device);
    if (dev >= 0 && !bvh) return fail(ctx, RVPT_HIP_ERR_INVALID, "bind on a brute-force context from a device pointer: its binding is kept on the host, pass a host array");
    const uint64_t n_records = 3ull * n_tris;
    uint32_t max_bone = 0;
    uint64_t max_pos = 0;
    if (dev < 0) {
        for (uint64_t r = 0; r < n_records; ++r)
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t b = skin[r].bone[j];
                if (b >= RVPT_HIP_SKIN_MAX_BONES)
                    return fail(ctx, RVPT_HIP_ERR_INVALID, "bind: skin[%llu].bone[%u] = %u: a bone index lies below %u", static_cast<unsigned long long>(r), j, b, RVPT_HIP_SKIN_MAX_BONES);
                if (b > max_bone) max_bone = b, max_pos = r;
            }
    } else if (n_records) {
        size_t cap_words = ctx->d_skin_words ? 2 : 0;
        if (int rc = grow(ctx, ctx->d_skin_words, cap_words, 2, sizeof(unsigned long long))) return rc;
        if (!ctx->h_skin_words) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_skin_words), 2 * sizeof(unsigned long long)));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_skin_words, 0xFF, sizeof(unsigned long long), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_skin_words + 1, 0, sizeof(unsigned long long), ctx->stream));
        hipLaunchKernelGGL(rv::skin_check, dim3(static_cast<uint32_t>((n_records + 255u) / 256u)), dim3(256), 0, ctx->stream, reinterpret_cast<const uint4 *>(skin), n_records,
                           RVPT_HIP_SKIN_MAX_BONES, ctx->d_skin_words);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_skin_words, ctx->d_skin_words, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const unsigned long long bad = ctx->h_skin_words[0], top = ctx->h_skin_words[1];
        if (bad != ~0ull) {
            const uint64_t r = bad >> 2;
            const uint32_t j = static_cast<uint32_t>(bad & 3u);
            uint32_t value = 0;
            if (r < n_records) HIP_TRY(ctx, hipMemcpy(&value, &skin[r].bone[j], sizeof value, hipMemcpyDeviceToHost));
            return fail(ctx, RVPT_HIP_ERR_INVALID, "bind: skin[%llu].bone[%u] = %u: a bone index lies below %u", static_cast<unsigned long long>(r), j, value, RVPT_HIP_SKIN_MAX_BONES);
        }
        max_bone = static_cast<uint32_t>(top >> 32), max_pos = 0xFFFFFFFFull - (top & 0xFFFFFFFFull);
    }
    // every refusal is behind: the copy (no frame reads d_skin, and every skin update has waited for its kernel)
    if (bvh) {
        if (int rc = grow(ctx, ctx->d_skin, ctx->cap_skin, 2 * n_records, sizeof(uint4))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_skin, skin, n_records * sizeof(rvpt_vertex_skin), dev >= 0 ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // caller may free its list on return
    } else {
        ctx->h_skin.assign(skin, skin + n_records);
    }
    ctx->have_skin = true;
    ctx->skin_max_bone = max_bone, ctx->skin_max_pos = max_pos;
    ctx->skin_bones = 0;
    ctx->err.clear();
    return RVPT_HIP_OK;
}

// one vertex through its four weighted matrices, the host form of rv::skin_vertices' arithmetic: q_j = pose_vertex_host(M[bone[j]], p), then per component
// ((w0 q0 + w1 q1) + w2 q2) + w3 q3, every product and sum rounded on its own (this file is compiled with -ffp-contract=off)
static void skin_vertex_host(const rvpt_bone *bones, const rvpt_vertex_skin &s, const float p[3], float out[3])
{
    float q[4][3];
    for (int j = 0; j < 4; ++j) pose_vertex_host(bones[s.bone[j]].m, p, q[j]);
    for (int i = 0; i < 3; ++i) {
        const float a = s.weight[0] * q[0][i], b = s.weight[1] * q[1][i], c = s.weight[2] * q[2][i], d = s.weight[3] * q[3][i];
        const float ab = a + b;
        const float abc = ab + c;
        out[i] = abc + d;
    }
}

// The SKIN UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): k matrices; every vertex of the stored scene is posed from the rest pose by the four weighted
// matrices its bound record names.  BVH contexts: the snapshot if the context holds no rest pose, rv::skin_vertices over every vertex quad, then the plain
// update form's tail (every box refitted).  Brute-force contexts skin on the host and run the plain form.  Everything is refused before anything is touched.
// (Two halves, as the pose update's, so that the guarded skin form can put its own refusal between them: skin_validate touches nothing stored, skin_execute
// refuses nothing a caller's arguments decide.)
struct SkinList {
    int dev = -1;  // the GPU whose memory holds the bones, -1: host memory
    bool bvh = false;
};

static int skin_validate(rvpt_hip_ctx *ctx, const rvpt_bone *bones, const rvpt_triangle *tris, size_t k, const rvpt_material *mats, size_t n_mats, SkinList *list)
{
    if (!ctx->have_scene) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update before any full upload_scene on this context: there is no scene to update");
    if (k == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update without bones");
    if (k > RVPT_HIP_SKIN_MAX_BONES) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update with %zu bones: at most %u", k, RVPT_HIP_SKIN_MAX_BONES);
    if (!bones) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update without a list: `nodes` points at one rvpt_bone per bone");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int dev = device_of_pointer(bones);
    if (reinterpret_cast<uintptr_t>(bones) % (dev >= 0 ? 16u : 4u))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update: the list at %p is not %u-byte aligned", static_cast<const void *>(bones), dev >= 0 ? 16u : 4u);
    if (tris) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update takes no triangles: the library skins the ones it holds (`tris` must be NULL)");
    if (mats || n_mats) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update takes no materials: it keeps the stored ones");
    if (!ctx->have_skin) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update before a bind: the stored scene has no weights (RVPT_HIP_NODES_BIND_SKIN)");
    if (k <= ctx->skin_max_bone)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update with %zu bones: the binding names bone %u (skin[%llu]), which needs %u", k, ctx->skin_max_bone,
                    static_cast<unsigned long long>(ctx->skin_max_pos), ctx->skin_max_bone + 1u);
    const size_t n_tris = ctx->n_tris;
    const bool bvh = is_bvh(ctx, n_tris);
    if (dev >= 0 && dev != ctx->device) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update: the bones are device memory of GPU %d, the context lives on GPU %d", dev, ctx->device);
    if (dev >= 0 && !bvh) return fail(ctx, RVPT_HIP_ERR_INVALID, "skin update of a brute-force context from a device pointer: it skins on the host, pass a host array");
    if (bvh && ctx->refit_levels.empty())  // (the laboratory's knob only, as in the plain form)
#if RVPT_HIP_LAB
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the breadth-first device layout of the tree: RVPT_HIP_BVH_CALLER_LAYOUT keeps the caller's, which has no level ranges");
#else
        return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the level ranges of the tree's device layout, which this context does not hold");
#endif
    list->dev = dev, list->bvh = bvh;
    return RVPT_HIP_OK;
}

static int skin_execute(rvpt_hip_ctx *ctx, const rvpt_bone *bones, size_t k, const SkinList &list)
{
    const size_t n_tris = ctx->n_tris;
    const int dev = list.dev;
    const bool bvh = list.bvh;

    if (!bvh) {  // the rest pose on the host, the skinned records through the plain form
        if (int rc0 = sync_all(ctx)) return rc0;
        std::vector<rvpt_triangle> skinned(n_tris);
        HIP_TRY(ctx, hipMemcpy(skinned.data(), ctx->d_tris, n_tris * sizeof(rvpt_triangle), hipMemcpyDeviceToHost));
        if (!ctx->have_rest) {
            ctx->h_rest.resize(12 * n_tris);
            for (size_t t = 0; t < n_tris; ++t) std::memcpy(&ctx->h_rest[12 * t], &skinned[t], offsetof(rvpt_triangle, mat_id));
            ctx->have_rest = true;
        }
        for (size_t t = 0; t < n_tris; ++t) {
            const float *r = &ctx->h_rest[12 * t];
            float *rows[3] = {skinned[t].vert0, skinned[t].vert1, skinned[t].vert2};
            for (int v = 0; v < 3; ++v) {
                skin_vertex_host(bones, ctx->h_skin[3 * t + v], r + 4 * v, rows[v]);
                rows[v][3] = r[4 * v + 3];
            }
        }
        const int rc0 = update_geometry(ctx, skinned.data(), n_tris);
        if (rc0 == RVPT_HIP_OK) ctx->err.clear();
        return rc0;
    }

    int rc;
    const uint32_t n = static_cast<uint32_t>(n_tris), kk = static_cast<uint32_t>(k);
    if ((rc = grow(ctx, ctx->d_bones, ctx->cap_bones, 3 * static_cast<size_t>(RVPT_HIP_SKIN_MAX_BONES), sizeof(float4)))) return rc;
    if (!ctx->have_rest && (rc = grow(ctx, ctx->d_rest, ctx->cap_rest, 3 * n_tris, sizeof(float4)))) return rc;
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight finish on the old geometry
    ctx->skin_bones = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bones, bones, k * sizeof(rvpt_bone), dev >= 0 ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    if (!ctx->have_rest) {  // the snapshot, as the pose update takes it: 48 of every 64 bytes of d_tris, device to device, in stored order
        HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_rest, offsetof(rvpt_triangle, mat_id), ctx->d_tris, sizeof(rvpt_triangle), offsetof(rvpt_triangle, mat_id), n_tris, hipMemcpyDeviceToDevice,
                                      ctx->stream));
        ctx->have_rest = true;
    }
    // a grid the device holds at once — as many work-groups per CU as their LDS allows, eight at the most —, each staging the matrices once and striding over the vertices
    const uint64_t skin_blocks = (3ull * n + rv::kSkinBlock - 1u) / rv::kSkinBlock;
    const uint64_t skin_per_cu = std::min<uint64_t>(8u, (160u * 1024u) / (k * sizeof(rvpt_bone) + 512u));
    const uint32_t skin_grid = static_cast<uint32_t>(std::min<uint64_t>(skin_blocks, static_cast<uint64_t>(std::max(ctx->num_cus, 1)) * skin_per_cu));
    hipLaunchKernelGGL(rv::skin_vertices, dim3(skin_grid), dim3(rv::kSkinBlock), k * sizeof(rvpt_bone), ctx->stream, ctx->d_rest,
                       ctx->d_skin, ctx->d_bones, kk, n, ctx->have_perm ? ctx->d_perm : nullptr, ctx->d_tris);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = update_geometry_tail(ctx, true, nullptr, n_tris))) {  // (a host `bones` is read by the copy above until the stream has been waited for)
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    ctx->skin_bones = kk;
    ctx->err.clear();
    return RVPT_HIP_OK;
}

static int update_geometry_skin(rvpt_hip_ctx *ctx, const rvpt_bone *bones, const rvpt_triangle *tris, size_t k, const rvpt_material *mats, size_t n_mats)
{
    SkinList list;
    if (int rc = skin_validate(ctx, bones, tris, k, mats, n_mats, &list)) return rc;
    return skin_execute(ctx, bones, k, list);
}

// The GUARDED SKIN UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h): the skin update — every box refitted —, then the cost of the stored tree, then, with a
// limit, once the cost has grown past limit x base cost, the rebuild tail of the guarded pose update: the skinned triangles and the rest pose through the old
// permutation into the caller's order, the build, the rest pose through the new permutation back.  The binding stays where it is, in the caller's order; the
// next skin update reads it through the new permutation and poses from the same rest pose through the same weights.  permille: 0 (report only) or
// 1000 .. 65535, checked by the caller.  Brute-force contexts hold no tree: the plain skin form.
static int update_geometry_skin_guarded(rvpt_hip_ctx *ctx, const rvpt_bone *bones, const rvpt_triangle *tris, size_t k, const rvpt_material *mats, size_t n_mats, uint32_t permille)
{
    // the skin form's own refusals come first, in its words and its order; then the one refusal of this form, before anything of the stored scene is touched
    SkinList list;
    if (int rc = skin_validate(ctx, bones, tris, k, mats, n_mats, &list)) return rc;
    if (!list.bvh) return skin_execute(ctx, bones, k, list);
    if (permille != 0 && ctx->built_by == rvpt_hip_ctx::kBuiltByCaller)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded skin update with a limit after an ordinary upload_scene: the tree is the caller's, the library has no builder to rebuild it by (report only, limit 0, is legal)");
    if (int rc = skin_execute(ctx, bones, k, list)) return rc;
    double cost = 0.0;
    bool have = false;
    if (int rc = device_tree_cost(ctx, &cost, &have)) return rc;
    const double base = ctx->base_cost;
    if (permille == 0 || !have || !ctx->have_cost || !ctx->have_perm || !(cost > static_cast<double>(permille) / 1000.0 * base)) {
        fail(ctx, RVPT_HIP_OK, "guarded skin update: cost %.17g, base cost %.17g, limit %u permille: refitted", cost, base, permille);
        return RVPT_HIP_OK;
    }
    return rebuild_keeping_rest(ctx, "skin", cost, base, permille);
}

// The GUARDED UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h; BVH contexts): the update form, then the cost of the refitted tree, then — with a limit,
// once the cost has grown past limit x base cost — a rebuild by the builder that made the stored tree, from the moved triangles carried back into the
// caller's order.  permille: 0 (report only) or 1000 .. 65535, checked by the caller.
static int update_geometry_guarded(rvpt_hip_ctx *ctx, const rvpt_triangle *tris, size_t n_tris, uint32_t permille)
{
    // the update form's own refusals come first and in its words; then the one refusal of this form, before anything of the stored scene is touched
    if (ctx->have_scene && n_tris == ctx->n_tris && permille != 0 && ctx->built_by == rvpt_hip_ctx::kBuiltByCaller)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded update with a limit after an ordinary upload_scene: the tree is the caller's, the library has no builder to rebuild it by (report only, limit 0, is legal)");
    if (int rc = update_geometry(ctx, tris, n_tris)) return rc;
    double cost = 0.0;
    bool have = false;
    if (int rc = device_tree_cost(ctx, &cost, &have)) return rc;
    const double base = ctx->base_cost;
    static const char *const kNames[] = {"", "lbvh", "ploc", "sah"};
    if (permille == 0 || !have || !ctx->have_cost || !(cost > static_cast<double>(permille) / 1000.0 * base)) {
        fail(ctx, RVPT_HIP_OK, "guarded update: cost %.17g, base cost %.17g, limit %u permille: refitted", cost, base, permille);
        return RVPT_HIP_OK;
    }
    // the rebuild: d_tris holds the moved vertices beside the stored mat_id rows, in leaf order; d_carry receives them in the caller's order.  A buffer of
    // its own: the build reads its source until its last gather and writes d_tris, d_prep and its scratch meanwhile
    const uint32_t n = static_cast<uint32_t>(n_tris);
    const int built_by = ctx->built_by;
    if (int rc = grow(ctx, ctx->d_carry, ctx->cap_carry, n_tris * 4u, sizeof(float4))) return rc;
    hipLaunchKernelGGL(rv::carry_back_triangles, dim3(static_cast<uint32_t>((4ull * n + 255u) / 256u)), dim3(256), 0, ctx->stream, ctx->d_tris, ctx->d_perm, n, ctx->d_carry);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = build_scene_on_device(ctx, reinterpret_cast<const rvpt_triangle *>(ctx->d_carry), n_tris, ctx->host_mats.data(), ctx->host_mats.size(), built_by == rvpt_hip_ctx::kBuiltPloc,
                                       built_by == rvpt_hip_ctx::kBuiltSah))
        return rc;  // the build form's rule: its message, and no scene after anything but a bad material index (which stored rows cannot hold)
    fail(ctx, RVPT_HIP_OK, "guarded update: cost %.17g, base cost %.17g, limit %u permille: rebuilt (%s), new base cost %.17g", cost, base, permille, kNames[built_by], ctx->base_cost);
    return RVPT_HIP_OK;
}

}  // namespace

static int upload_scene_other_forms(rvpt_hip_ctx *ctx, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t n_mats);

int rvpt_hip_upload_scene(rvpt_hip_ctx *ctx, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris,
                          size_t n_tris, const rvpt_material *mats, size_t n_mats)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    // the POSE UPDATE: the count RVPT_HIP_NODES_UPDATE_POSE, `nodes` then points at n_tris rvpt_part_move records and `tris` is NULL (the form checks that itself)
    if (n_nodes == RVPT_HIP_NODES_UPDATE_POSE) return update_geometry_pose(ctx, reinterpret_cast<const rvpt_part_move *>(nodes), tris, n_tris, mats, n_mats);
    // the BIND and the SKIN UPDATE: `nodes` points at three rvpt_vertex_skin records per triangle, or at n_tris rvpt_bone matrices; both keep the rest pose
    if (n_nodes == RVPT_HIP_NODES_BIND_SKIN) return bind_skin(ctx, reinterpret_cast<const rvpt_vertex_skin *>(nodes), tris, n_tris, mats, n_mats);
    if (n_nodes == RVPT_HIP_NODES_UPDATE_SKIN) return update_geometry_skin(ctx, reinterpret_cast<const rvpt_bone *>(nodes), tris, n_tris, mats, n_mats);
    // the GUARDED POSE UPDATE: the same arguments and a count of the band RVPT_HIP_NODES_UPDATE_POSE_GUARDED(permille) lies in.  It keeps the rest pose, through a
    // rebuild too; only a rebuild that failed, and so left no scene, has dropped it
    if ((size_t)0 - n_nodes >= 0x200000u && (size_t)0 - n_nodes < 0x300000u) {
        const size_t permille = (size_t)0 - n_nodes - 0x200000u;
        if (permille != 0 && (permille < 1000u || permille > 65535u))
            return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded pose update: the limit is 0 (report only) or 1000 .. 65535 permille, got %zu", permille);
        const int rc = update_geometry_pose_guarded(ctx, reinterpret_cast<const rvpt_part_move *>(nodes), tris, n_tris, mats, n_mats, static_cast<uint32_t>(permille));
        if (!ctx->have_scene) drop_skin(ctx);  // (a rebuild that failed)
        return rc;
    }
    // the GUARDED SKIN UPDATE: the skin update's arguments and a count of the band RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(permille) lies in.  It keeps the rest pose and
    // the binding, through a rebuild too; only a rebuild that failed, and so left no scene, has dropped them
    if ((size_t)0 - n_nodes >= 0x300000u && (size_t)0 - n_nodes < 0x400000u) {
        const size_t permille = (size_t)0 - n_nodes - 0x300000u;
        if (permille != 0 && (permille < 1000u || permille > 65535u))
            return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded skin update: the limit is 0 (report only) or 1000 .. 65535 permille, got %zu", permille);
        const int rc = update_geometry_skin_guarded(ctx, reinterpret_cast<const rvpt_bone *>(nodes), tris, n_tris, mats, n_mats, static_cast<uint32_t>(permille));
        if (!ctx->have_scene) drop_skin(ctx);  // (a rebuild that failed)
        return rc;
    }
    // the update forms keep the skin update's binding; a full upload and a build form the caller asks for drop it, and so does any call that leaves no scene
    const bool update_form = n_nodes == RVPT_HIP_NODES_UPDATE_SPARSE || (n_tris > 0 && !nodes && n_nodes == 0 && !mats && n_mats == 0) ||
                             (!nodes && (size_t)0 - n_nodes >= 0x10000u && (size_t)0 - n_nodes < 0x110000u);
    const int rc = upload_scene_other_forms(ctx, nodes, n_nodes, tris, n_tris, mats, n_mats);
    if ((rc == RVPT_HIP_OK && !update_form) || !ctx->have_scene) drop_skin(ctx);
    // the rest pose of the pose update is the stored vertices as the last successful call of any OTHER form left them: the next pose update snapshots afresh
    if (rc == RVPT_HIP_OK || !ctx->have_scene) ctx->have_rest = false;
    return rc;
}

static int upload_scene_other_forms(rvpt_hip_ctx *ctx, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t n_mats)
{
    if ((n_tris && !tris) || (n_mats && !mats)) return fail(ctx, RVPT_HIP_ERR_INVALID, "NULL scene array");
    if (n_tris > 0x3FFFFFFFull) return fail(ctx, RVPT_HIP_ERR_INVALID, "too many triangles");
    // the SPARSE UPDATE: the count RVPT_HIP_NODES_UPDATE_SPARSE, `nodes` then points at n_tris indices (n_tris == 0 arrives here too: the form says so itself)
    if (n_nodes == RVPT_HIP_NODES_UPDATE_SPARSE) return update_geometry_sparse(ctx, reinterpret_cast<const uint32_t *>(nodes), tris, n_tris, mats, n_mats);
    // the UPDATE FORM: triangles without nodes and without materials (as a full upload it could never succeed: no material index fits n_mats == 0)
    if (n_tris > 0 && !nodes && n_nodes == 0 && !mats && n_mats == 0) return update_geometry(ctx, tris, n_tris);
    // the GUARDED UPDATE: no nodes and a count of the band RVPT_HIP_NODES_UPDATE_GUARDED(permille) lies in.  Brute-force contexts hold no tree: the plain update form
    if (!nodes && (size_t)0 - n_nodes >= 0x10000u && (size_t)0 - n_nodes < 0x110000u) {
        const size_t permille = (size_t)0 - n_nodes - 0x10000u;
        if (permille != 0 && (permille < 1000u || permille > 65535u))
            return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded update: the limit is 0 (report only) or 1000 .. 65535 permille, got %zu", permille);
        if (mats || n_mats) return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded update takes no materials: it keeps the stored ones");
        if (n_tris == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded update without triangles");
        if (is_bvh(ctx, n_tris)) return update_geometry_guarded(ctx, tris, n_tris, static_cast<uint32_t>(permille));
        const int rc = update_geometry(ctx, tris, n_tris);
        if (rc == RVPT_HIP_OK) ctx->err.clear();
        return rc;
    }
    // the BUILD FORM: no nodes and the sentinel count.  BVH contexts build the tree on the device; brute-force contexts ignore nodes and n_nodes as ever
    if (!nodes && (n_nodes == RVPT_HIP_NODES_BUILD || n_nodes == RVPT_HIP_NODES_BUILD_PLOC || n_nodes == RVPT_HIP_NODES_BUILD_SAH)) {
        if (is_bvh(ctx, n_tris)) return build_scene_on_device(ctx, tris, n_tris, mats, n_mats, n_nodes == RVPT_HIP_NODES_BUILD_PLOC, n_nodes == RVPT_HIP_NODES_BUILD_SAH);
        n_nodes = 0;
    }
    // an EMPTY scene has no tree (RVPT::initialize with no triangles): every ray misses whatever the traversal, and the
    // frame kernels of a BVH context then run the brute-force instance over zero triangles (choose_launch)
    const bool bvh = is_bvh(ctx, n_tris);
    uint32_t bvh_height_tmp = 0;
    // materials[int(mat_id.x)] (intersection.glsl:398) must stay inside the buffer
    for (size_t i = 0; i < n_tris; ++i) {
        const float m = tris[i].mat_id[0];
        if (!(m >= 0.0f) || static_cast<size_t>(static_cast<int>(m)) >= n_mats)
            return fail(ctx, RVPT_HIP_ERR_INVALID, "triangle %zu: material index %g outside [0,%zu)", i, static_cast<double>(m), n_mats);
    }
    if (bvh) {
        if (!nodes || n_nodes == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "BVH context needs nodes");
        for (size_t i = 0; i < n_nodes; ++i) {
            const rvpt_bvh_node &nd = nodes[i];
            if (nd.primitive_count > 0) {
                if (static_cast<uint64_t>(nd.first_child_or_primitive) + nd.primitive_count > n_tris)
                    return fail(ctx, RVPT_HIP_ERR_INVALID, "node %zu: leaf range outside the triangle buffer", i);
            } else if (static_cast<uint64_t>(nd.first_child_or_primitive) + 1 >= n_nodes) {
                return fail(ctx, RVPT_HIP_ERR_INVALID, "node %zu: child index outside the node buffer", i);
            }
        }
        // height of the tree = what the traversal stack must hold; also rejects cycles
        std::vector<std::pair<uint32_t, uint32_t>> work{{0u, 1u}};
        uint32_t height = 0;
        size_t visited = 0;
        while (!work.empty()) {
            const auto [idx, depth] = work.back();
            work.pop_back();
            if (++visited > n_nodes) return fail(ctx, RVPT_HIP_ERR_INVALID, "BVH is not a tree (node reachable twice)");
            height = std::max(height, depth);
            if (nodes[idx].primitive_count == 0) {
                work.emplace_back(nodes[idx].first_child_or_primitive, depth + 1);
                work.emplace_back(nodes[idx].first_child_or_primitive + 1, depth + 1);
            }
        }
        // the reference's uint stack[64] holds its sentinel + one push per inner node of a root-to-leaf path: a leaf may sit
        // on level 64 (root = level 1); deeper trees overflow it there (undefined) and are rejected here
        if (height > rv::kBvhStackDepth)
            return fail(ctx, RVPT_HIP_ERR_INVALID, "BVH height %u exceeds the %u levels the reference's 64-entry traversal stack can walk (intersection.glsl:363-372)", height, rv::kBvhStackDepth);
        bvh_height_tmp = height;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight still read the old scene
    int rc;
    ctx->have_sparse_maps = ctx->have_inv_perm = ctx->have_surface_inv = false;  // the topology the sparse update's maps were made for is being replaced
    if ((rc = grow(ctx, ctx->d_tris, ctx->cap_tris, n_tris, sizeof(rvpt_triangle)))) return rc;
    if ((rc = grow(ctx, ctx->d_prep, ctx->cap_prep, n_tris, sizeof(rvpt_triangle)))) return rc;
    if ((rc = grow(ctx, ctx->d_mat_index, ctx->cap_mat_index, n_tris, sizeof(uint32_t)))) return rc;
    if ((rc = grow(ctx, ctx->d_unit_n, ctx->cap_unit_n, n_tris, sizeof(float4)))) return rc;
    if ((rc = grow(ctx, ctx->d_mats, ctx->cap_mats, n_mats, sizeof(rvpt_material)))) return rc;
    if (n_tris) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_tris, tris, n_tris * sizeof(rvpt_triangle), hipMemcpyHostToDevice, ctx->stream));
    if (n_mats) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_mats, mats, n_mats * sizeof(rvpt_material), hipMemcpyHostToDevice, ctx->stream));
    if (n_mats) {  // the device copy's data.w = 1 / ior ("Unused" in the reference: structs.glsl:31)
        hipLaunchKernelGGL(rv::prepare_materials, dim3((static_cast<uint32_t>(n_mats) + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_mats, static_cast<uint32_t>(n_mats));
        HIP_TRY(ctx, hipGetLastError());
    }
    std::vector<rvpt_bvh_node> device_nodes;  // must outlive the async copy below (stream is synchronised before return)
    size_t n_device_nodes = 0;
    std::vector<std::pair<uint32_t, uint32_t>> levels;  // the levels of the breadth-first layout as device index ranges (rvpt_hip_ctx::refit_levels)
    if (bvh) {
        // Device layout of the tree (traversal order and results are unchanged): breadth-first, root at 0, slot 1
        // unused, every sibling pair on an even index = one 64-byte line, upper levels first.
        if (ctx->knobs.bvh_caller_layout) {
            device_nodes.assign(nodes, nodes + n_nodes);
            if (device_nodes.size() < 2) device_nodes.resize(2);  // the kernels copy at least the root's 64-byte line into LDS
        } else {
            device_nodes.resize(n_nodes + 1);
            std::memset(device_nodes.data(), 0, device_nodes.size() * sizeof(rvpt_bvh_node));
            std::vector<std::pair<uint32_t, uint32_t>> queue;  // (caller index, device index), FIFO
            queue.reserve(n_nodes);
            queue.emplace_back(0u, 0u);
            uint32_t next_pair = 2;
            size_t level_end = 0;  // queue entries below this belong to the levels recorded so far
            for (size_t head = 0; head < queue.size(); ++head) {
                if (head == level_end) {  // the level above has been expanded: what the queue holds from here on is exactly the next level
                    levels.emplace_back(queue[head].second, queue.back().second + 1u);
                    level_end = queue.size();
                }
                const auto [src, dst] = queue[head];
                rvpt_bvh_node nd = nodes[src];
                if (nd.primitive_count == 0) {
                    const uint32_t child = nd.first_child_or_primitive;
                    nd.first_child_or_primitive = next_pair;
                    queue.emplace_back(child, next_pair);
                    queue.emplace_back(child + 1, next_pair + 1);
                    next_pair += 2;
                }
                device_nodes[dst] = nd;
            }
        }
        n_device_nodes = device_nodes.size();
        if ((rc = grow(ctx, ctx->d_nodes, ctx->cap_nodes, n_device_nodes, sizeof(rvpt_bvh_node)))) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_nodes, device_nodes.data(), n_device_nodes * sizeof(rvpt_bvh_node), hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = launch_prepare_triangles(ctx, n_tris))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // caller may free its arrays on return
    ctx->n_tris = n_tris;
    ctx->n_mats = n_mats;
    ctx->n_nodes = bvh ? n_device_nodes : 0;
    ctx->bvh_height = bvh_height_tmp;
    ctx->refit_levels = std::move(levels);
    ctx->bvh_head_shift = 0;
    if (bvh) {  // can a node's (first, count) pair ride in one stack word?  indices below 2^shift, leaf sizes below 2^(32 - shift)
        uint32_t shift = 1, max_count = 0;
        while (shift < 31 && (1ull << shift) <= std::max(n_device_nodes, n_tris)) shift += 1;
        for (size_t i = 0; i < n_nodes; ++i) max_count = std::max(max_count, nodes[i].primitive_count);
        if (static_cast<uint64_t>(max_count) < (1ull << (32 - shift))) ctx->bvh_head_shift = shift;
    }
    ctx->n_wide = 0;
    ctx->wide_stack_levels = 0;
    ctx->have_perm = false;  // the triangles are in the leaf order of the caller's tree: the update form takes that order
    if (bvh && !ctx->knobs.bvh_caller_layout) {  // the 4-wide form of the tree (breadth-first device layout: children of node i at first, first + 1)
        uint32_t need = 0;
        std::vector<uint32_t> kid_map;
        const std::vector<float> wide = rv::build_wide_nodes(device_nodes.data(), device_nodes.size(), ctx->bvh_head_shift, need, &kid_map);
        if (!wide.empty() && need <= 4096u && wide.size() / 32 < rv::kWideMaxNodes) {
            const size_t n_wide = wide.size() / 32;
            if ((rc = grow(ctx, ctx->d_wide, ctx->cap_wide, n_wide * 8, sizeof(float4)))) return rc;
            HIP_TRY(ctx, hipMemcpy(ctx->d_wide, wide.data(), wide.size() * sizeof(float), hipMemcpyHostToDevice));
            if ((rc = grow(ctx, ctx->d_wide_map, ctx->cap_wide_map, kid_map.size(), sizeof(uint32_t)))) return rc;
            HIP_TRY(ctx, hipMemcpy(ctx->d_wide_map, kid_map.data(), kid_map.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            ctx->n_wide = n_wide;
            ctx->wide_stack_levels = need;
        }
    }
    if ((rc = derive_bounce_state(ctx, bvh, tris, n_tris))) return rc;
    ctx->base_cost = 0.0, ctx->have_cost = false;
    if (bvh && (rc = device_tree_cost(ctx, &ctx->base_cost, &ctx->have_cost))) return rc;  // the base cost of the guarded update
    ctx->built_by = rvpt_hip_ctx::kBuiltByCaller;
    if (bvh) ctx->host_mats.assign(mats, mats + n_mats);
    ctx->scene_gen += 1;  // the slots' screen rectangles belong to the old scene
    ctx->have_scene = true;
    return RVPT_HIP_OK;
}

int rvpt_hip_set_frame(rvpt_hip_ctx *ctx, const rvpt_render_settings *s, const rvpt_camera_data *cam)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!s || !cam) return fail(ctx, RVPT_HIP_ERR_INVALID, "NULL settings/camera");
    if (s->aa < 1) return fail(ctx, RVPT_HIP_ERR_INVALID, "aa must be >= 1 (got %d)", s->aa);
    // every render mode (0..9, anything else = integrator_Hart) and camera mode (0, 1, anything else = spherical)
    // of compute_pass.comp:68-118 is implemented
    ctx->settings = *s;
    ctx->camera = *cam;
    ctx->have_frame = true;
    return RVPT_HIP_OK;
}

namespace {

// The packet kernel's camera records and screen rectangles for this camera: made on the slot's stream, in front of the frame kernel, when the slot's buffers hold another
// camera's.  With `sky`, the slot's sky bits, list and count for the same camera too (sky_blocks, sky_list), the count copied to the host behind them (sky_ready).
static int update_rects(rvpt_hip_ctx *ctx, int slot, hipStream_t tstream, const rv::FrameParams &p, bool sky)
{
    if (ctx->n_tris > ctx->rects_cap[slot]) {
        HIP_TRY(ctx, hipStreamSynchronize(tstream));
        if (ctx->d_rects[slot]) HIP_TRY(ctx, hipFree(ctx->d_rects[slot]));
        if (ctx->d_cam_records[slot]) HIP_TRY(ctx, hipFree(ctx->d_cam_records[slot]));
        ctx->d_rects[slot] = nullptr;
        ctx->d_cam_records[slot] = nullptr;
        ctx->rects_cap[slot] = 0;
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_rects[slot]), ctx->n_tris * sizeof(uint2)));
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_cam_records[slot]), ctx->n_tris * sizeof(float4)));
        ctx->rects_cap[slot] = ctx->n_tris;
        ctx->rects_valid[slot] = false;
    }
    rvpt_hip_ctx::RectKey key{};
    key.camera = ctx->camera;
    key.scene_gen = ctx->scene_gen;
    if (!ctx->rects_valid[slot] || std::memcmp(&key, &ctx->rects_key[slot], sizeof(key)) != 0) {
        const uint32_t n = static_cast<uint32_t>(ctx->n_tris);
        hipLaunchKernelGGL(rv::camera_rects, dim3((n + 63) / 64), dim3(64), 0, tstream, p, ctx->d_rects[slot], ctx->d_cam_records[slot]);
        HIP_TRY(ctx, hipGetLastError());
        ctx->rects_key[slot] = key;
        ctx->rects_valid[slot] = true;
        ctx->sky_valid[slot] = false;
    }
    if (sky && !ctx->sky_valid[slot]) {
        const uint32_t n_blocks = ctx->n_work / 64u;  // (n_work: whole 16 x 16 tiles)
        if (!ctx->d_sky_bits[slot]) {  // (all five made, then published together: a failure part way leaves the slot without a list, never with half of one)
            uint32_t *bits = nullptr, *count = nullptr;
            uint2 *list = nullptr;
            hipEvent_t ready = nullptr, read = nullptr;
            hipError_t e = hipMalloc(reinterpret_cast<void **>(&bits), static_cast<size_t>((n_blocks + 31u) / 32u) * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&list), static_cast<size_t>(n_blocks) * sizeof(uint2));
            if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&count), sizeof(uint32_t));
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&read, hipEventDisableTiming);
            if (e != hipSuccess) {
                if (bits) (void)hipFree(bits);
                if (list) (void)hipFree(list);
                if (count) (void)hipFree(count);
                if (ready) (void)hipEventDestroy(ready);
                return fail(ctx, RVPT_HIP_ERR_HIP, "sky list buffers -> %s", hipGetErrorString(e));
            }
            ctx->d_sky_bits[slot] = bits, ctx->d_sky_list[slot] = list, ctx->d_sky_count[slot] = count;
            ctx->sky_ready[slot] = ready, ctx->sky_read[slot] = read;
        }
        if (!ctx->h_sky_count) HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->h_sky_count), rvpt_hip_ctx::kMaxSlots * sizeof(uint32_t)));
        if (ctx->sky_read_used[slot]) HIP_TRY(ctx, hipStreamWaitEvent(tstream, ctx->sky_read[slot], 0));  // the last blend that reads the slot's old bits
        hipLaunchKernelGGL(rv::sky_blocks, dim3((n_blocks + 255u) / 256u), dim3(256), 0, tstream, p, ctx->d_rects[slot], n_blocks, ctx->d_sky_bits[slot]);
        hipLaunchKernelGGL(rv::sky_list, dim3(1), dim3(1024), 0, tstream, p, ctx->d_sky_bits[slot], n_blocks, ctx->d_sky_list[slot], ctx->d_sky_count[slot]);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_sky_count + slot, ctx->d_sky_count[slot], sizeof(uint32_t), hipMemcpyDeviceToHost, tstream));
        HIP_TRY(ctx, hipEventRecord(ctx->sky_ready[slot], tstream));
        ctx->sky_valid[slot] = true;
    }
    return 0;
}

// one launch covering n_frames consecutive frames starting at settings.current_frame
static int dispatch_launch(rvpt_hip_ctx *ctx, uint32_t n_frames)
{
    const int slots = slots_for(ctx, n_frames);  // launches in flight for this kind of launch; no drain when it changes: a slot's
    if (ctx->next_slot >= slots) ctx->next_slot = 0;  // reuse waits for its own last blend, and the blends are enqueued in dispatch order
    const int slot = ctx->next_slot;
    ctx->next_slot = (slot + 1) % slots;
    ctx->last_slots = slots;
    hipStream_t tstream = ctx->overlap ? ctx->trace_stream[slot] : ctx->stream;
    const int buf = slot * rvpt_hip_ctx::kBufsPerSlot + ctx->slot_parity[slot];
    ctx->slot_parity[slot] ^= 1;
    if (ctx->overlap && n_frames > ctx->samples_cap[buf]) {
        // first batch of this size: grow the sample buffers of all the slots this kind of launch rotates over now (one drain),
        // not one buffer per later launch
        if (int rc = sync_all(ctx)) return rc;
        for (int i = 0; i < slots * rvpt_hip_ctx::kBufsPerSlot; ++i) {
            if (ctx->samples_cap[i] >= n_frames) continue;
            HIP_TRY(ctx, hipFree(ctx->d_samples[i]));
            ctx->d_samples[i] = nullptr;
            ctx->samples_cap[i] = 0;
            const size_t bytes = static_cast<size_t>(n_frames) * ctx->slot_quads * sizeof(rv::SampleRGB);
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_samples[i]), bytes));
            // lanes of partial edge tiles outside the image never store; blend_accumulate folds the padding into the
            // accumulator padding, which is part of the tile buffer handed to gathers: keep it defined (as create does).
            // ON THE SLOT'S OWN STREAM: the streams are non-blocking, a null-stream hipMemset is not ordered against them
            // and would race with the frame kernel launched next (it did: 1 case in 1 500 of tools/fuzz_parity.py)
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_samples[i], 0, bytes, ctx->trace_stream[i / rvpt_hip_ctx::kBufsPerSlot]));
            ctx->samples_cap[i] = n_frames;
        }
    }
    rv::FrameParams p{};
    fill_frame_params(ctx, slot, p, buf);
    p.n_work = n_frames * ctx->n_work;
    // is anything of this context still running?  (a finished or never used stream answers hipSuccess)  Only the HBM-resident BVH launches of >= 16 frames act on the
    // answer (choose_launch); a one-frame brute-force launch does not pay six stream queries for it.  (After the growth above: its drain makes the answer "idle".)
    bool lone = false;
    if (ctx->overlap && is_bvh(ctx, ctx->n_tris) && n_frames >= 16u) {
        lone = true;
        for (int i = 0; i < ctx->n_slots && lone; ++i)
            if (ctx->slot_used[i] && hipStreamQuery(ctx->trace_stream[i]) != hipSuccess) lone = false;
        (void)hipGetLastError();  // hipErrorNotReady is an answer, not an error
    }
    // the knob's test form (RVPT_HIP_PACKETS_SKY_LIST=2): the slot's rectangles and sky list for this camera first, waited for, so that a first batched launch takes the listed path
    if (ctx->knobs.packets_sky_list == 2 && n_frames >= 4u && ctx->settings.aa == 1 && !is_bvh(ctx, ctx->n_tris) && ctx->n_tris > 0 && ctx->n_tris <= rv::kResidentMaxTris) {
        if (int rc = update_rects(ctx, slot, tstream, p, true)) return rc;
        HIP_TRY(ctx, hipEventSynchronize(ctx->sky_ready[slot]));
    }
    Launch launch{};
    if (int rc = choose_launch(ctx, p, lone, slots, slot, launch)) return rc;
    if (launch.variant == Variant::BrutePackets) {
        if (int rc = update_rects(ctx, slot, tstream, p, launch.sky_wanted)) return rc;
        if (launch.cull_bits & kCullRects) p.rects = ctx->d_rects[slot];
        p.cam_records = ctx->d_cam_records[slot];
    }
    if (has_global_stack(launch.variant) && p.stack_levels > p.stack_lds_levels) {  // global part of the traversal stack, one column per thread and level
        const size_t words = static_cast<size_t>(2) * (p.stack_levels - p.stack_lds_levels) * launch.grid * rv::kBlock;
        if (words > ctx->stack_overflow_cap[slot]) {
            HIP_TRY(ctx, hipStreamSynchronize(tstream));
            if (ctx->d_stack_overflow[slot]) HIP_TRY(ctx, hipFree(ctx->d_stack_overflow[slot]));
            ctx->d_stack_overflow[slot] = nullptr;
            ctx->stack_overflow_cap[slot] = 0;
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_stack_overflow[slot]), words * sizeof(uint32_t)));
            ctx->stack_overflow_cap[slot] = words;
        }
        p.stack_overflow = ctx->d_stack_overflow[slot];
    }
    if (!ctx->knobs.timeline_path.empty()) {
        const size_t words = static_cast<size_t>(p.n_waves) * 16;  // 8 per wave + 8 more for the instrumented BVH build's load counts
        if (words > ctx->timeline_words) {
            if (ctx->d_timeline) HIP_TRY(ctx, hipFree(ctx->d_timeline));
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->d_timeline), words * 8));
            ctx->timeline_words = words;
        }
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_timeline, 0, words * 8, tstream));
        p.timeline = ctx->d_timeline;
    }
    ctx->last_grid = launch.grid;
    ctx->last_lds = static_cast<uint32_t>(launch.lds);
    ctx->last_variant = static_cast<uint32_t>(launch.variant);
    ctx->last_cull = launch.cull_bits;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (ctx->timing) {
        if (ctx->pending.size() >= 4096) {
            int rc = drain_timing(ctx);
            if (rc) return rc;
        }
        if (!ctx->spare.empty()) {
            ev0 = ctx->spare.back().first;
            ev1 = ctx->spare.back().second;
            ctx->spare.pop_back();
        } else {
            HIP_TRY(ctx, hipEventCreate(&ev0));
            HIP_TRY(ctx, hipEventCreate(&ev1));
        }
    }
    // this sample buffer is free once the blend of the launch that last wrote it — two launches back on this stream — has consumed it
    if (ctx->overlap && ctx->buf_used[buf]) HIP_TRY(ctx, hipStreamWaitEvent(tstream, ctx->blend_done[buf], 0));
    ctx->buf_used[buf] = true;
    ctx->slot_used[slot] = true;
    if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ev0, tstream));
    if (launch.listed && launch.work.run_frames != 0u)
        hipLaunchKernelGGL(rv::trace_brute_packets_aa1_culls_listed_runs, dim3(launch.grid), dim3(rv::kBlock), launch.lds, tstream, p, launch.work);
    else if (launch.listed)
        hipLaunchKernelGGL(rv::trace_brute_packets_aa1_culls_listed, dim3(launch.grid), dim3(rv::kBlock), launch.lds, tstream, p, launch.work);
    else
        hipLaunchKernelGGL(launch.kernel, dim3(launch.grid), dim3(rv::kBlock), launch.lds, tstream, p);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->timing) {
        HIP_TRY(ctx, hipEventRecord(ev1, tstream));
        ctx->pending.emplace_back(ev0, ev1);
    }
    if (ctx->overlap) {  // the temporal blend of this frame, after its samples and after every earlier blend
        HIP_TRY(ctx, hipEventRecord(ctx->trace_done[slot], tstream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->trace_done[slot], 0));
        if (launch.listed) {  // (the sky's samples were never made: the blend makes them)
            hipLaunchKernelGGL(rv::blend_accumulate_sky, dim3((ctx->n_work + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_samples[buf], n_frames, ctx->d_sky_bits[slot], p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipEventRecord(ctx->sky_read[slot], ctx->stream));
            ctx->sky_read_used[slot] = true;
        } else {
            hipLaunchKernelGGL(rv::blend_accumulate, dim3((ctx->n_work + 255) / 256), dim3(256), 0, ctx->stream, ctx->d_samples[buf],
                               ctx->d_accum, ctx->n_work, n_frames, p.frame, p.quantize);
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ctx->blend_done[buf], ctx->stream));
    }
    ctx->seq += 1;
    return RVPT_HIP_OK;
}

// The work / exit counters of a slot are reset by the last wave of each launch.  If a launch failed or the device reported
// an error, that may not have happened and every later frame on the slot would silently skip claimed work: zero them
// (best effort — the context may be beyond repair, the caller gets the original error either way).
static void reset_counters_after_error(rvpt_hip_ctx *ctx)
{
    if (!ctx || !ctx->d_counter) return;
    (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    (void)hipMemsetAsync(ctx->d_counter, 0, ctx->n_slots * rv::kCounterWords * sizeof(unsigned long long), ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);  // the context's streams are non-blocking: nothing may start before the counters are zero
}

static int dispatch_checked(rvpt_hip_ctx *ctx, uint32_t n_frames)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!ctx->have_scene) return fail(ctx, RVPT_HIP_ERR_INVALID, "dispatch before upload_scene");
    if (!ctx->have_frame) return fail(ctx, RVPT_HIP_ERR_INVALID, "dispatch before set_frame");
    if (n_frames == 0 || n_frames > RVPT_HIP_MAX_FRAMES_PER_DISPATCH)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "n_frames = %u (1..%u)", n_frames, RVPT_HIP_MAX_FRAMES_PER_DISPATCH);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->n_work == 0) return RVPT_HIP_OK;  // this rank owns no tile
    // one launch covers as many frames as fit 2^31 work items; without frames in flight there are no sample buffers
    // to batch into and the frames go one by one (same result, dispatch order)
    const uint64_t max_items = 0x7FFFFFFFull;
    const uint32_t per_launch = ctx->overlap ? std::max<uint32_t>(1, std::min<uint32_t>(n_frames, static_cast<uint32_t>(max_items / ctx->n_work))) : 1u;
    const uint32_t base = ctx->settings.current_frame;
    int rc = RVPT_HIP_OK;
    for (uint32_t done = 0; done < n_frames && rc == RVPT_HIP_OK; done += per_launch) {
        ctx->settings.current_frame = base + done;
        rc = dispatch_launch(ctx, std::min(per_launch, n_frames - done));
    }
    ctx->settings.current_frame = base;
    if (rc == RVPT_HIP_ERR_HIP) reset_counters_after_error(ctx);
    return rc;
}

}  // namespace

int rvpt_hip_dispatch(rvpt_hip_ctx *ctx) { return dispatch_checked(ctx, 1); }

int rvpt_hip_dispatch_frames(rvpt_hip_ctx *ctx, uint32_t n_frames) { return dispatch_checked(ctx, n_frames); }

int rvpt_hip_wait(rvpt_hip_ctx *ctx)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = sync_all(ctx);
    if (rc == RVPT_HIP_ERR_HIP) reset_counters_after_error(ctx);
    if (rc == RVPT_HIP_OK && ctx->debug_checks && ctx->d_counter) {
        // the word after each slot's exited-wave counter: set by a wave that pushed past the top of the traversal stack the host sized (rvpt_device.h:
        // report_stack_overflow) — the clamp kept the kernel inside its memory, the image is wrong; never silently
        bool overflow = false;
        for (int i = 0; i < ctx->n_slots; ++i) {
            unsigned long long word = 0;
            unsigned long long *at = ctx->d_counter + static_cast<size_t>(i) * rv::kCounterWords + rv::kShardStride * rv::kClaimShards + 1;
            HIP_TRY(ctx, hipMemcpy(&word, at, sizeof(word), hipMemcpyDeviceToHost));
            if (word != 0) {
                overflow = true;
                HIP_TRY(ctx, hipMemset(at, 0, sizeof(word)));
            }
        }
        if (overflow) return fail(ctx, RVPT_HIP_ERR_INVALID, "BVH traversal stack overflow: a lane pushed past the %u levels the host sized for this tree — the frame is wrong", ctx->wide_stack_levels ? ctx->wide_stack_levels : ctx->bvh_height);
    }
    return rc;
}

int rvpt_hip_query(rvpt_hip_ctx *ctx)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    for (int i = 0; i <= ctx->n_slots; ++i) {
        hipStream_t st = (i < ctx->n_slots) ? ctx->trace_stream[i] : ctx->stream;
        hipError_t e = hipStreamQuery(st);
        if (e == hipErrorNotReady) return 1;
        if (e != hipSuccess) return fail(ctx, RVPT_HIP_ERR_HIP, "hipStreamQuery -> %s", hipGetErrorString(e));
    }
    return 0;
}

int rvpt_hip_wait_for(rvpt_hip_ctx *ctx, uint64_t timeout_ns)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::nanoseconds(timeout_ns);
    for (;;) {
        const int q = rvpt_hip_query(ctx);
        if (q < 0) reset_counters_after_error(ctx);
        if (q <= 0) return q == 0 ? sync_all(ctx) : q;  // done (collect timing events) or error
        if (std::chrono::steady_clock::now() >= deadline) return 1;
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}


namespace {

// How long a collective (or the communicator's bootstrap) may take before it is reported as failed: RVPT_HIP_COMM_TIMEOUT_S, default
// 120 s.  A peer that never enters a collective would otherwise leave this rank waiting forever inside a stream.
static double comm_timeout_s()
{
    const char *e = getenv("RVPT_HIP_COMM_TIMEOUT_S");
    const double v = e ? atof(e) : 0.0;
    return v > 0.0 ? v : 120.0;
}

// Wait for `stream` — which carries a collective — at most comm_timeout_s().  On a timeout the communicator is aborted (a
// collective that did not complete leaves it unusable) and every context of the group loses it: later collectives report "no
// communicator" instead of waiting again.
static int ensure_comm_stream(rvpt_hip_ctx *ctx, rvpt_hip_ctx *m)
{
    if (m->comm_stream && !m->comm_stream_lost) return RVPT_HIP_OK;
    m->comm_stream = nullptr;  // (a lost stream is leaked on purpose: destroying it would wait for the collective that never completes)
    m->comm_stream_lost = false;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&m->comm_stream, hipStreamNonBlocking));
    return RVPT_HIP_OK;
}

static int sync_collective(rvpt_hip_ctx *ctx, rvpt_hip_ctx *member, const char *what)
{
    const auto t0 = std::chrono::steady_clock::now();
    const auto deadline = t0 + std::chrono::duration<double>(comm_timeout_s());
    for (;;) {
        const hipError_t e = hipStreamQuery(member->comm_stream);
        if (e == hipSuccess) return RVPT_HIP_OK;
        if (e != hipErrorNotReady) return fail(ctx, RVPT_HIP_ERR_HIP, "%s: hipStreamQuery -> %s", what, hipGetErrorString(e));
        const auto now = std::chrono::steady_clock::now();
        if (now >= deadline) break;
        if (now - t0 > std::chrono::milliseconds(2)) std::this_thread::sleep_for(std::chrono::microseconds(50));  // spin first: a warm gather takes ~0.1 ms
    }
    const std::vector<rvpt_hip_ctx *> group = ctx->local_group.empty() ? std::vector<rvpt_hip_ctx *>{ctx} : ctx->local_group;
    bool aborted = true;
    for (rvpt_hip_ctx *m : group) {
        if (m->comm && !(rccl().CommAbort && rccl().CommAbort(m->comm) == ncclSuccess)) aborted = false;
        m->comm = nullptr;
        m->comm_stream_lost = true;  // whatever the abort achieved, nothing of this context ever waits on that stream again
    }
    for (rvpt_hip_ctx *m : group) m->local_group.clear();
    return fail(ctx, RVPT_HIP_ERR_COMM, "%s timed out after %.0f s (rank %u of %u: did every rank enter the collective?); the communicator was %s and its stream "
                "abandoned — rendering, read-back of this rank's tiles and wait are unaffected (they never share a stream with a collective)",
                what, comm_timeout_s(), ctx->tile_rank, ctx->tile_world, aborted ? "aborted" : "dropped (ncclCommAbort unavailable or failed)");
}

// Gather of per-tile radiance to rank 0: every rank sends its tile-linear accumulator (one slot of slot_quads
// pixels, the payload the renderer already keeps resident), rank 0 receives tile_world slots — grouped ncclSend / ncclRecv,
// so over xGMI each peer uses its own direct link to the root — and un-tiles them into a row-major frame.
// `frame_dev` (rank 0): width*height float4 on ctx's device, or NULL to receive without un-tiling (rank 0 found its own arguments
// invalid but still takes part: a rank that returned early would leave its peers waiting).  Single-process groups are driven from
// rank 0's context.  Everything that can fail LOCALLY (arguments, allocations, the frames in flight) is dealt with before the group
// is opened; a failure after that point aborts the communicator (sync_collective).
static int gather_to_root(rvpt_hip_ctx *ctx, float4 *frame_dev)
{
    const Rccl &n = rccl();
    if (!ctx->comm) return fail(ctx, RVPT_HIP_ERR_COMM, "context has no communicator (rvpt_hip_comm_init / rvpt_hip_comm_init_all)");
    const bool single_process = !ctx->local_group.empty();
    if (single_process && ctx->tile_rank != 0)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "in a single-process group the collective is driven through rank 0's context");
    const size_t floats = ctx->slot_quads * 4;
    std::vector<rvpt_hip_ctx *> members = single_process ? ctx->local_group : std::vector<rvpt_hip_ctx *>{ctx};
    // local work first.  A local failure here is reported AFTER the exchange: this rank still posts its send / receives (of
    // whatever the accumulator holds), because its peers are already on their way into the group call.
    int local_rc = RVPT_HIP_OK;
    std::string local_err;
    for (rvpt_hip_ctx *m : members) {  // everything rendered and blended before the accumulator leaves
        if (hipSetDevice(m->device) != hipSuccess || sync_all(m) != RVPT_HIP_OK) {
            if (local_rc == RVPT_HIP_OK) local_rc = RVPT_HIP_ERR_HIP, local_err = m->err.empty() ? "hipSetDevice failed" : m->err;
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->tile_rank == 0 && !ctx->d_gather) {
        if (hipMalloc(reinterpret_cast<void **>(&ctx->d_gather), static_cast<size_t>(ctx->tile_world) * floats * sizeof(float)) != hipSuccess) {
            // without a receive buffer this rank cannot take part; the peers' sends time out on their side (sync_collective)
            ctx->d_gather = nullptr;
            return fail(ctx, RVPT_HIP_ERR_HIP, "gather buffer of %zu bytes could not be allocated", static_cast<size_t>(ctx->tile_world) * floats * sizeof(float));
        }
    }
    for (rvpt_hip_ctx *m : members) {
        HIP_TRY(ctx, hipSetDevice(m->device));
        if (int rc = ensure_comm_stream(ctx, m)) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RCCL_TRY(ctx, n.GroupStart());
    ncclResult_t first_error = ncclSuccess;  // a group that was opened is always closed, whatever a call inside it returned
    auto in_group = [&](ncclResult_t r) {
        if (r != ncclSuccess && first_error == ncclSuccess) first_error = r;
    };
    for (rvpt_hip_ctx *m : members) {
        if (m->tile_rank == 0)
            for (uint32_t r = 0; r < m->tile_world && first_error == ncclSuccess; ++r)
                in_group(n.Recv(reinterpret_cast<float *>(m->d_gather) + static_cast<size_t>(r) * floats, floats, ncclFloat, static_cast<int>(r), m->comm, m->comm_stream));
        if (first_error == ncclSuccess) in_group(n.Send(m->d_accum, floats, ncclFloat, 0, m->comm, m->comm_stream));
    }
    in_group(n.GroupEnd());
    if (first_error != ncclSuccess) return fail(ctx, RVPT_HIP_ERR_COMM, "gather of per-tile radiance -> %s", n.GetErrorString(first_error));
    if (ctx->tile_rank == 0 && frame_dev != nullptr) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        const dim3 blk(64, 4), grd((ctx->width + 63) / 64, (ctx->height + 3) / 4);
        hipLaunchKernelGGL(rv::untile_rgba32f, grd, blk, 0, ctx->comm_stream, ctx->d_gather, ctx->slot_quads, ctx->tile_world, ctx->width, ctx->height,
                           ctx->tiles_x, frame_dev);
        HIP_TRY(ctx, hipGetLastError());
    }
    for (rvpt_hip_ctx *m : members) {
        HIP_TRY(ctx, hipSetDevice(m->device));
        if (int rc = sync_collective(ctx, m, "gather of per-tile radiance")) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (local_rc != RVPT_HIP_OK) return fail(ctx, local_rc, "%s (the gather itself completed)", local_err.c_str());
    return RVPT_HIP_OK;
}

void drop_comm(rvpt_hip_ctx *ctx)
{
    // A single-process group dissolves as a whole with its first member to go: every member's communicator is destroyed
    // here, so that a later collective on a surviving context reports "no communicator" instead of waiting for a peer
    // that no longer exists.
    const std::vector<rvpt_hip_ctx *> group = ctx->local_group.empty() ? std::vector<rvpt_hip_ctx *>{ctx} : ctx->local_group;
    for (rvpt_hip_ctx *m : group) {
        if (m->comm && rccl().ok) {
            (void)hipSetDevice(m->device);
            (void)rccl().CommDestroy(m->comm);
        }
        m->comm = nullptr;
        m->local_group.clear();
    }
    (void)hipSetDevice(ctx->device);
}

}  // namespace

int rvpt_hip_comm_unique_id(void *id_out, size_t id_bytes)
{
    if (!id_out || id_bytes < RVPT_HIP_COMM_ID_BYTES) return fail(nullptr, RVPT_HIP_ERR_INVALID, "id buffer must hold %d bytes", RVPT_HIP_COMM_ID_BYTES);
    static_assert(sizeof(ncclUniqueId) == RVPT_HIP_COMM_ID_BYTES, "RVPT_HIP_COMM_ID_BYTES");
    if (!rccl().ok) return fail(nullptr, RVPT_HIP_ERR_COMM, "%s", rccl().why.c_str());
    ncclUniqueId id;
    RCCL_TRY(nullptr, rccl().GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof id);
    return RVPT_HIP_OK;
}

int rvpt_hip_comm_init(rvpt_hip_ctx *ctx, const void *unique_id, size_t id_bytes)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!unique_id || id_bytes < RVPT_HIP_COMM_ID_BYTES) return fail(ctx, RVPT_HIP_ERR_INVALID, "unique id must be %d bytes", RVPT_HIP_COMM_ID_BYTES);
    if (ctx->comm) return fail(ctx, RVPT_HIP_ERR_INVALID, "context already has a communicator");
    if (!rccl().ok) return fail(ctx, RVPT_HIP_ERR_COMM, "%s", rccl().why.c_str());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    // ncclCommInitRank blocks until every rank of the group has joined; a rank that never comes (it failed before this call, it was
    // handed another id) must not hang the others: the bootstrap runs on a helper thread and is given comm_timeout_s()
    struct Boot {
        std::mutex m;
        std::condition_variable cv;
        bool done = false, abandoned = false;  // abandoned: the caller gave up waiting; a communicator that arrives late is the helper's to destroy
        ncclResult_t result = ncclSuccess;
        ncclComm_t comm = nullptr;
    };
    auto boot = std::make_shared<Boot>();
    const int device = ctx->device, world = static_cast<int>(ctx->tile_world), rank = static_cast<int>(ctx->tile_rank);
    std::thread([boot, id, device, world, rank] {
        ncclComm_t c = nullptr;
        ncclResult_t r = (hipSetDevice(device) == hipSuccess) ? rccl().CommInitRank(&c, world, id, rank) : static_cast<ncclResult_t>(1);
        bool late = false;
        {
            std::lock_guard<std::mutex> lock(boot->m);
            boot->result = r;
            boot->comm = c;
            boot->done = true;
            late = boot->abandoned;
            boot->cv.notify_all();
        }
        // the bootstrap completed after rvpt_hip_comm_init had timed out: nobody will ever use this communicator, and its peers believe this rank
        // joined — abort it (their next collective then fails at once instead of waiting out the full timeout) or at least destroy it
        if (late && r == ncclSuccess && c != nullptr) {
            if (!(rccl().CommAbort && rccl().CommAbort(c) == ncclSuccess)) (void)rccl().CommDestroy(c);
        }
    }).detach();
    {
        std::unique_lock<std::mutex> lock(boot->m);
        if (!boot->cv.wait_for(lock, std::chrono::duration<double>(comm_timeout_s()), [&] { return boot->done; })) {
            boot->abandoned = true;
            return fail(ctx, RVPT_HIP_ERR_COMM, "ncclCommInitRank (rank %d of %d) did not complete within %.0f s: not every rank joined with this id", rank, world, comm_timeout_s());
        }
        if (boot->result != ncclSuccess) return fail(ctx, RVPT_HIP_ERR_COMM, "ncclCommInitRank (rank %d of %d) -> %s", rank, world, rccl().GetErrorString(boot->result));
        ctx->comm = boot->comm;
    }
    return RVPT_HIP_OK;
}

int rvpt_hip_comm_init_all(rvpt_hip_ctx *const *ctxs, int n)
{
    if (!ctxs || n < 1) return fail(nullptr, RVPT_HIP_ERR_INVALID, "no contexts");
    std::vector<int> devices(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        rvpt_hip_ctx *c = ctxs[i];
        if (!c) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctxs[%d] is NULL", i);
        if (c->tile_world != static_cast<uint32_t>(n) || c->tile_rank != static_cast<uint32_t>(i))
            return fail(c, RVPT_HIP_ERR_INVALID, "ctxs[%d] is tile %u of %u: the group must list ranks 0..%d of %d in order", i, c->tile_rank, c->tile_world, n - 1, n);
        if (c->comm) return fail(c, RVPT_HIP_ERR_INVALID, "ctxs[%d] already has a communicator", i);
        if (c->width != ctxs[0]->width || c->height != ctxs[0]->height) return fail(c, RVPT_HIP_ERR_INVALID, "ctxs[%d]: image size differs", i);
        devices[static_cast<size_t>(i)] = c->device;
    }
    if (!rccl().ok) return fail(ctxs[0], RVPT_HIP_ERR_COMM, "%s", rccl().why.c_str());
    std::vector<ncclComm_t> comms(static_cast<size_t>(n), nullptr);
    RCCL_TRY(ctxs[0], rccl().CommInitAll(comms.data(), n, devices.data()));
    std::vector<rvpt_hip_ctx *> group(ctxs, ctxs + n);
    for (int i = 0; i < n; ++i) {
        ctxs[i]->comm = comms[static_cast<size_t>(i)];
        ctxs[i]->local_group = group;
    }
    return RVPT_HIP_OK;
}

int rvpt_hip_comm_info(rvpt_hip_ctx *ctx, int *n_ranks, int *rank, int *rccl_version)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (n_ranks) *n_ranks = 0;
    if (rank) *rank = -1;
    if (rccl_version) *rccl_version = 0;
    if (!ctx->comm) return fail(ctx, RVPT_HIP_ERR_COMM, "context has no communicator (rvpt_hip_comm_init / rvpt_hip_comm_init_all)");
    const Rccl &n = rccl();
    // asked of RCCL itself, not echoed from the context: "did RCCL see N ranks?" is what a scaling record must be able to answer
    if (n_ranks && n.CommCount) RCCL_TRY(ctx, n.CommCount(ctx->comm, n_ranks));
    if (rank && n.CommUserRank) RCCL_TRY(ctx, n.CommUserRank(ctx->comm, rank));
    if (rccl_version && n.GetVersion) RCCL_TRY(ctx, n.GetVersion(rccl_version));
    return RVPT_HIP_OK;
}

int rvpt_hip_comm_destroy(rvpt_hip_ctx *ctx)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    drop_comm(ctx);  // a single-process group dissolves as a whole
    return RVPT_HIP_OK;
}

int rvpt_hip_comm_barrier(rvpt_hip_ctx *ctx)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!ctx->comm) return fail(ctx, RVPT_HIP_ERR_COMM, "context has no communicator (rvpt_hip_comm_init / rvpt_hip_comm_init_all)");
    const bool single_process = !ctx->local_group.empty();
    if (single_process && ctx->tile_rank != 0)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "in a single-process group the collective is driven through rank 0's context");
    const Rccl &n = rccl();
    std::vector<rvpt_hip_ctx *> members = single_process ? ctx->local_group : std::vector<rvpt_hip_ctx *>{ctx};
    for (rvpt_hip_ctx *m : members) {  // this rank's own work first, and the one float the all-reduce carries
        HIP_TRY(ctx, hipSetDevice(m->device));
        if (int rc = sync_all(m)) return rc;
        if (int rc = ensure_comm_stream(ctx, m)) return rc;
        if (!m->d_barrier) {
            HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&m->d_barrier), 256));
            HIP_TRY(ctx, hipMemsetAsync(m->d_barrier, 0, 256, m->comm_stream));
        }
    }
    RCCL_TRY(ctx, n.GroupStart());
    ncclResult_t first_error = ncclSuccess;
    for (rvpt_hip_ctx *m : members) {
        const ncclResult_t r = n.AllReduce(m->d_barrier, m->d_barrier, 1, ncclFloat, ncclSum, m->comm, m->comm_stream);
        if (r != ncclSuccess && first_error == ncclSuccess) first_error = r;
    }
    {
        const ncclResult_t r = n.GroupEnd();
        if (r != ncclSuccess && first_error == ncclSuccess) first_error = r;
    }
    if (first_error != ncclSuccess) return fail(ctx, RVPT_HIP_ERR_COMM, "barrier -> %s", n.GetErrorString(first_error));
    for (rvpt_hip_ctx *m : members) {
        HIP_TRY(ctx, hipSetDevice(m->device));
        if (int rc = sync_collective(ctx, m, "barrier")) return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return RVPT_HIP_OK;
}

int rvpt_hip_gather(rvpt_hip_ctx *ctx, void *dst_dev_rgba32f)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (ctx->tile_rank == 0 && !dst_dev_rgba32f && ctx->comm) {  // rank 0's own mistake must not leave the peers waiting: take part, then report
        (void)gather_to_root(ctx, nullptr);
        return fail(ctx, RVPT_HIP_ERR_INVALID, "rank 0 needs a destination");
    }
    return gather_to_root(ctx, static_cast<float4 *>(dst_dev_rgba32f));
}

// rvpt_hip_read with a format of records, by `kind`: RVPT_HIP_FORMAT_RAY_HITS (include/rvpt_hip.h: RAY QUERIES), RVPT_HIP_FORMAT_RAY_PATHS (PATH QUERIES),
// RVPT_HIP_FORMAT_NEAREST_POINTS (NEAREST POINTS) or RVPT_HIP_FORMAT_SURFACE_POINTS (SURFACE POINTS).  `dst` holds dst_bytes / 48 records: rays in and hits —
// radiance — out, points in and nearest points out, or (prim, u, v) in and the point, material and normal of the stored mesh out.
// The forms share everything but the kernels and the first out byte: the checks, the pointer's classification, the staging of host records (only a record's
// out fields travel back: its third float4, for a point query its second and third).  LOCAL: no communicator is touched.  Everything is checked before
// anything is written; on success ctx->err stays as it was.  No event is recorded: RVPT_HIP_TIMING does not see a query.
// `path_mode` (RecordKind::Paths only): the integrator of the call, 0 .. 9 — RVPT_HIP_FORMAT_RAY_PATHS is mode 9, RVPT_HIP_FORMAT_RAY_PATHS_MODE(m) is mode m.
// `hits` (RecordKind::Rays only): 0 for RVPT_HIP_FORMAT_RAY_HITS and for RVPT_HIP_FORMAT_RAY_HITS_NEAREST(1), which is the same call; k for RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k), k > 1 (K-NEAREST RAY QUERIES) — `dst` then holds groups of
// k records, one ray each, and the plan and the launch count groups; everything else, the staging and the copy back of every record's out quad included, is
// per record as before.
enum class RecordKind { Rays, Paths, Points, Surface };
static int query_records(rvpt_hip_ctx *ctx, void *dst, size_t dst_bytes, const RecordKind kind, const uint32_t path_mode = rv::kPathModeKajiya, const uint32_t hits = 0)
{
    const bool paths = kind == RecordKind::Paths, points = kind == RecordKind::Points, surface = kind == RecordKind::Surface;
    const char *what = surface ? "surface" : (points ? "point" : (paths ? "path" : "ray"));
    const char *record = surface ? "rvpt_surface_point" : (points ? "rvpt_point_hit" : (paths ? "rvpt_ray_path" : "rvpt_ray_hit"));
    const size_t out_offset = surface ? offsetof(rvpt_surface_point, point) : (points ? offsetof(rvpt_point_hit, closest) : offsetof(rvpt_ray_hit, t));  // where a record's out fields begin
    if (hits && dst_bytes % (sizeof(rvpt_ray_hit) * hits))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "ray query with k = %u: dst_bytes %zu is not a multiple of the %zu bytes of a group of k rvpt_ray_hit", hits, dst_bytes,
                    sizeof(rvpt_ray_hit) * hits);
    if (dst_bytes % sizeof(rvpt_ray_hit))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "%s query: dst_bytes %zu is not a multiple of the %zu bytes of a %s", what, dst_bytes, sizeof(rvpt_ray_hit), record);
    if (!ctx->have_scene) return fail(ctx, RVPT_HIP_ERR_INVALID, "%s query before any full upload_scene on this context: there is no scene to ask", what);
    const size_t n = dst_bytes / sizeof(rvpt_ray_hit);
    if (n == 0) return RVPT_HIP_OK;
    if (!dst) return fail(ctx, RVPT_HIP_ERR_INVALID, "dst is NULL");
    if (n > 0xFFFFFFFFull) return fail(ctx, RVPT_HIP_ERR_INVALID, "%s query: %zu records, at most 2^32 - 1 per call", what, n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool device_dst = false;
    if (int rc = classify_frame_pointer(ctx, dst, "dst", &device_dst)) return rc;
    if (device_dst && reinterpret_cast<uintptr_t>(dst) % 16u)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "dst is device memory at %p: %s records on the device need 16-byte alignment", dst, what);

    rv::PathScene path_scene{};
    rv::QueryScene &scene = path_scene.walk;
    const bool bvh = is_bvh(ctx, ctx->n_tris);
    scene.kind = !bvh ? rv::QueryKind::Brute : (ctx->n_wide > 0 && ctx->bvh_head_shift != 0 ? rv::QueryKind::Wide : rv::QueryKind::Binary);
    scene.prep = ctx->d_prep, scene.nodes = ctx->d_nodes, scene.wide = ctx->d_wide;
    scene.perm = ctx->have_perm ? ctx->d_perm : nullptr;
    scene.n_tris = static_cast<uint32_t>(ctx->n_tris), scene.n_wide = static_cast<uint32_t>(ctx->n_wide), scene.head_shift = ctx->bvh_head_shift;
    scene.stack_levels = scene.kind == rv::QueryKind::Wide ? ctx->wide_stack_levels : bvh_stack_levels(ctx);
    path_scene.mat_index = ctx->d_mat_index, path_scene.unit_n = ctx->d_unit_n, path_scene.mats = ctx->d_mats;
    rv::NearestScene nearest{};  // a point query reads the vertex rows and the binary nodes, whichever form the ray walks of this context take
    nearest.brute = !bvh;
    nearest.tris = ctx->d_tris, nearest.nodes = ctx->d_nodes, nearest.perm = scene.perm;
    nearest.n_tris = scene.n_tris, nearest.n_nodes = static_cast<uint32_t>(ctx->n_nodes), nearest.stack_levels = bvh_stack_levels(ctx);
    const uint32_t groups_of = hits ? hits : 1u;  // records per ray
    rv::QueryPlan plan{};
    if (points)
        HIP_TRY(ctx, rv::nearest_plan(nearest, static_cast<uint32_t>(n), ctx->num_cus, &plan));
    else if (paths)
        HIP_TRY(ctx, rv::path_plan(path_scene, static_cast<uint32_t>(n), ctx->num_cus, path_mode, &plan));
    else if (!surface)  // (a surface read is one record per lane and no walk: no plan, no stack)
        HIP_TRY(ctx, rv::query_plan(scene, static_cast<uint32_t>(n / groups_of), ctx->num_cus, &plan, groups_of));
    if (int rc = rvpt_hip_wait(ctx)) return rc;  // every read implies it; frames in flight still read the scene, and the buffers below may be regrown
    if (int rc = grow(ctx, ctx->d_query_scratch, ctx->cap_query_scratch, 64u + plan.stack_words, sizeof(uint32_t))) return rc;
    void *records = dst;
    if (!device_dst) {
        if (int rc = grow(ctx, ctx->d_query_stage, ctx->cap_query_stage, dst_bytes, 1)) return rc;
        records = ctx->d_query_stage;
        HIP_TRY(ctx, hipMemcpyAsync(records, dst, dst_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    if (surface) {
        // caller's index -> stored row on a context with a permutation: an inverse of the read side's own, under its own flag (d_inv_perm and have_inv_perm
        // are the update forms', and the laboratory read-back shows them)
        const bool permuted = ctx->have_perm && ctx->n_tris > 0;
        if (permuted && !ctx->have_surface_inv) {
            if (int rc = grow(ctx, ctx->d_surface_inv, ctx->cap_surface_inv, ctx->n_tris, sizeof(uint32_t))) return rc;
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_surface_inv, 0xFF, ctx->n_tris * sizeof(uint32_t), ctx->stream));
            hipLaunchKernelGGL(rv::sparse_invert_permutation, dim3((scene.n_tris + 255u) / 256u), dim3(256), 0, ctx->stream, ctx->d_perm, scene.n_tris, ctx->d_surface_inv);
            HIP_TRY(ctx, hipGetLastError());
            ctx->have_surface_inv = true;
        }
        rv::SurfaceScene mesh{};
        mesh.tris = ctx->d_tris, mesh.unit_n = ctx->d_unit_n, mesh.mat_index = ctx->d_mat_index;
        mesh.inv_perm = permuted ? ctx->d_surface_inv : nullptr, mesh.n_tris = scene.n_tris;
        HIP_TRY(ctx, rv::surface_launch(ctx->stream, mesh, records, static_cast<uint32_t>(n)));
    } else if (points)
        HIP_TRY(ctx, rv::nearest_launch(ctx->stream, nearest, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n)));
    else if (paths)
        HIP_TRY(ctx, rv::path_launch(ctx->stream, path_scene, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n), path_mode));
    else
        HIP_TRY(ctx, rv::query_launch(ctx->stream, scene, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n / groups_of), groups_of));
    if (!device_dst)  // only the out fields travel back: the in fields of a host record are never written either
        HIP_TRY(ctx, hipMemcpy2DAsync(static_cast<unsigned char *>(dst) + out_offset, sizeof(rvpt_ray_hit), ctx->d_query_stage + out_offset, sizeof(rvpt_ray_hit),
                                      sizeof(rvpt_ray_hit) - out_offset, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // device records: the caller may read them from any stream of its own on return
    return RVPT_HIP_OK;
}

// rvpt_hip_read with RVPT_HIP_FORMAT_TRIANGLES (include/rvpt_hip.h: TRIANGLES): the stored rows of d_tris, all 64 bytes of each, in the update order of the
// context — d_tris itself without a permutation (one copy), the row scatter out[perm[s]] = tris[s] with one (straight into a device `dst`; for a host `dst`
// into the queries' staging buffer, then one copy).  Nothing is recomputed.  LOCAL.  Everything is checked before anything is written; on success ctx->err
// stays as it was.
static int read_triangles(rvpt_hip_ctx *ctx, void *dst, size_t dst_bytes)
{
    if (!ctx->have_scene) return fail(ctx, RVPT_HIP_ERR_INVALID, "triangle read before any full upload_scene on this context: there is no scene to read");
    const size_t need = ctx->n_tris * sizeof(rvpt_triangle);
    if (need == 0) return RVPT_HIP_OK;  // the empty scene: nothing to write, dst may be NULL
    if (!dst) return fail(ctx, RVPT_HIP_ERR_INVALID, "dst is NULL");
    if (dst_bytes < need) return fail(ctx, RVPT_HIP_ERR_SIZE, "dst holds %zu bytes, the %zu stored triangles need %zu", dst_bytes, ctx->n_tris, need);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool device_dst = false;
    if (int rc = classify_frame_pointer(ctx, dst, "dst", &device_dst)) return rc;
    if (device_dst && reinterpret_cast<uintptr_t>(dst) % 16u)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "dst is device memory at %p: triangle rows on the device need 16-byte alignment", dst);
    if (int rc = rvpt_hip_wait(ctx)) return rc;  // every read implies it; the staging buffer below may be regrown
    if (!ctx->have_perm) {
        HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->d_tris, need, device_dst ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    } else if (device_dst) {
        HIP_TRY(ctx, rv::surface_scatter_rows(ctx->stream, ctx->d_tris, ctx->d_perm, static_cast<uint32_t>(ctx->n_tris), dst));
    } else {
        if (int rc = grow(ctx, ctx->d_query_stage, ctx->cap_query_stage, need, 1)) return rc;
        HIP_TRY(ctx, rv::surface_scatter_rows(ctx->stream, ctx->d_tris, ctx->d_perm, static_cast<uint32_t>(ctx->n_tris), ctx->d_query_stage));
        HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->d_query_stage, need, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // a device dst: the caller may read it from any stream of its own on return
    return RVPT_HIP_OK;
}

int rvpt_hip_read(rvpt_hip_ctx *ctx, int format, void *dst, size_t dst_bytes)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (format >= RVPT_HIP_FORMAT_RAY_PATHS_MODE(0) && format <= RVPT_HIP_FORMAT_RAY_PATHS_MODE(9))  // a path query by integrator (mode 9 is RVPT_HIP_FORMAT_RAY_PATHS itself); local as well
        return query_records(ctx, dst, dst_bytes, RecordKind::Paths, static_cast<uint32_t>(format - RVPT_HIP_FORMAT_RAY_PATHS_MODE(0)));
    if (format == RVPT_HIP_FORMAT_RAY_HITS_NEAREST(1)) return query_records(ctx, dst, dst_bytes, RecordKind::Rays);  // k = 1 IS format 2, its messages included
    if (format > RVPT_HIP_FORMAT_RAY_HITS_NEAREST(1) && format <= static_cast<int>(RVPT_HIP_FORMAT_RAY_HITS_NEAREST(RVPT_HIP_RAY_MAX_HITS)))  // the k nearest hits of a ray; local as well
        return query_records(ctx, dst, dst_bytes, RecordKind::Rays, rv::kPathModeKajiya, static_cast<uint32_t>(format) - RVPT_HIP_FORMAT_RAY_HITS_NEAREST(0u));
    if (format == RVPT_HIP_FORMAT_TRIANGLES) return read_triangles(ctx, dst, dst_bytes);  // local as well
    if (format == RVPT_HIP_FORMAT_SURFACE_POINTS) return query_records(ctx, dst, dst_bytes, RecordKind::Surface);
    if (format == RVPT_HIP_FORMAT_RAY_HITS || format == RVPT_HIP_FORMAT_RAY_PATHS || format == RVPT_HIP_FORMAT_NEAREST_POINTS)  // local even with a communicator: every rank holds the whole scene
        return query_records(ctx, dst, dst_bytes,
                             format == RVPT_HIP_FORMAT_NEAREST_POINTS ? RecordKind::Points : (format == RVPT_HIP_FORMAT_RAY_PATHS ? RecordKind::Paths : RecordKind::Rays));
    const bool collective = ctx->comm != nullptr;  // partitioned image with a communicator: gather to rank 0, which gets the frame
    if (collective && ctx->tile_rank != 0 && ctx->local_group.empty()) return gather_to_root(ctx, nullptr);  // peers only send
    const size_t px = static_cast<size_t>(ctx->width) * ctx->height;
    const size_t need = px * (format == RVPT_HIP_FORMAT_RGBA32F ? 16 : 4);
    // rank 0's arguments.  In a collective read its peers are already sending: a bad argument here is reported AFTER this rank
    // has taken part in the exchange (receiving without un-tiling), never by leaving them in the group call.
    int arg_rc = RVPT_HIP_OK;
    if (!dst)
        arg_rc = fail(ctx, RVPT_HIP_ERR_INVALID, "dst is NULL");
    else if (format != RVPT_HIP_FORMAT_RGBA32F && format != RVPT_HIP_FORMAT_RGBA8_UNORM)
        arg_rc = fail(ctx, RVPT_HIP_ERR_INVALID, "unknown format %d", format);
    else if (dst_bytes < need)
        arg_rc = fail(ctx, RVPT_HIP_ERR_SIZE, "dst holds %zu bytes, frame needs %zu", dst_bytes, need);
    if (arg_rc == RVPT_HIP_OK && hipSetDevice(ctx->device) != hipSuccess) arg_rc = fail(ctx, RVPT_HIP_ERR_HIP, "hipSetDevice failed");
    bool device_dst = false;  // dst is device memory of this GPU: the layout kernels write it in place, the frame never visits the host
    if (arg_rc == RVPT_HIP_OK) arg_rc = classify_frame_pointer(ctx, dst, "dst", &device_dst);
    if (arg_rc == RVPT_HIP_OK && (collective || !device_dst)) arg_rc = ensure_rowmajor(ctx);
    if (arg_rc != RVPT_HIP_OK) {
        if (collective) {
            const std::string keep = ctx->err;
            (void)gather_to_root(ctx, nullptr);
            ctx->err = keep;
        }
        return arg_rc;
    }
    int rc = RVPT_HIP_OK;
    if (collective) {
        if ((rc = gather_to_root(ctx, static_cast<float4 *>(ctx->d_rowmajor)))) return rc;
        if (device_dst) {  // the gathered frame leaves d_rowmajor for dst on the device: quantised on the way, or as it is (a byte copy: dst may be 4-byte aligned only)
            if (format == RVPT_HIP_FORMAT_RGBA8_UNORM) {
                hipLaunchKernelGGL(rv::quantize_rowmajor, dim3(static_cast<uint32_t>((px + 255) / 256)), dim3(256), 0, ctx->stream,
                                   static_cast<const float4 *>(ctx->d_rowmajor), static_cast<uint32_t>(px), static_cast<uint32_t *>(dst));
                HIP_TRY(ctx, hipGetLastError());
            } else {
                HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->d_rowmajor, need, hipMemcpyDeviceToDevice, ctx->stream));
            }
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return RVPT_HIP_OK;
        }
        const void *src = ctx->d_rowmajor;
        if (format == RVPT_HIP_FORMAT_RGBA8_UNORM) {
            if (!ctx->d_quant) HIP_TRY(ctx, hipMalloc(&ctx->d_quant, px * 4));
            hipLaunchKernelGGL(rv::quantize_rowmajor, dim3(static_cast<uint32_t>((px + 255) / 256)), dim3(256), 0, ctx->stream,
                               static_cast<const float4 *>(ctx->d_rowmajor), static_cast<uint32_t>(px), static_cast<uint32_t *>(ctx->d_quant));
            HIP_TRY(ctx, hipGetLastError());
            src = ctx->d_quant;
        }
        HIP_TRY(ctx, hipMemcpyAsync(dst, src, need, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return RVPT_HIP_OK;
    }
    const dim3 blk(64, 4), grd((ctx->width + 63) / 64, (ctx->height + 3) / 4);
    if (device_dst) {  // un-tiled (and quantised) straight into dst: no d_rowmajor, no second copy
        const bool as_rgba8 = format == RVPT_HIP_FORMAT_RGBA8_UNORM;
        if (as_rgba8 || reinterpret_cast<uintptr_t>(dst) % 16u == 0)  // (rgba8: 4-byte stores; RGBA32F: read_rowmajor stores a pixel as one float4)
            hipLaunchKernelGGL(rv::read_rowmajor, grd, blk, 0, ctx->stream, ctx->d_accum, ctx->width, ctx->height, ctx->tiles_x, ctx->tile_rank, ctx->tile_world, as_rgba8 ? 1 : 0, dst);
        else
            hipLaunchKernelGGL(rv::read_rowmajor_dwords, dim3((4u * ctx->width + 63) / 64, grd.y), blk, 0, ctx->stream, reinterpret_cast<const float *>(ctx->d_accum), ctx->width,
                               ctx->height, ctx->tiles_x, ctx->tile_rank, ctx->tile_world, static_cast<float *>(dst));
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the caller may read dst from any stream of its own on return
        return RVPT_HIP_OK;
    }
    hipLaunchKernelGGL(rv::read_rowmajor, grd, blk, 0, ctx->stream, ctx->d_accum, ctx->width, ctx->height, ctx->tiles_x,
                       ctx->tile_rank, ctx->tile_world, format == RVPT_HIP_FORMAT_RGBA8_UNORM ? 1 : 0, ctx->d_rowmajor);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(dst, ctx->d_rowmajor, need, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RVPT_HIP_OK;
}

int rvpt_hip_tile_buffer(rvpt_hip_ctx *ctx, void **device_ptr, size_t *bytes, size_t *max_tile_bytes)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (device_ptr) *device_ptr = ctx->d_accum;
    if (bytes) *bytes = static_cast<size_t>(ctx->n_work) * sizeof(float4);
    if (max_tile_bytes) *max_tile_bytes = static_cast<size_t>(owned_tiles(ctx->tiles_x * ctx->tiles_y, 0, ctx->tile_world)) * 256u * sizeof(float4);
    return RVPT_HIP_OK;
}

#if RVPT_HIP_LAB  // ---- include/rvpt_hip_lab.h: diagnostics of the arithmetic specification and of the exact culls; the laboratory build only
int rvpt_hip_selftest_div(int device_id, const float *a, const float *b, float *out, size_t n)
{
    if (!a || !b || !out) return fail(nullptr, RVPT_HIP_ERR_INVALID, "NULL array");
    if (n == 0) return RVPT_HIP_OK;
    if (n > (1u << 30)) return fail(nullptr, RVPT_HIP_ERR_INVALID, "n too large");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    float *d = nullptr;
    HIP_TRY(nullptr, hipMalloc(reinterpret_cast<void **>(&d), 3 * n * sizeof(float)));
    hipError_t e = hipMemcpy(d, a, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, b, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rv::selftest_div_dots, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, nullptr, d, d + n, d + 2 * n, static_cast<uint32_t>(n));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(nullptr, RVPT_HIP_ERR_HIP, "selftest_div -> %s", hipGetErrorString(e));
    return RVPT_HIP_OK;
}

int rvpt_camera_rects(const float *prepared, size_t n_tris, const rvpt_camera_data *cam, uint32_t width, uint32_t height, uint32_t *rects_out)
{
    if ((n_tris && !prepared) || !cam || !rects_out) return RVPT_HIP_ERR_INVALID;
    // FrameParams' view of the camera block (fill_frame_params): columns 0..2, the origin, aspect, 1 / tan(vfov / 2)
    float c[12];
    for (int col = 0; col < 3; ++col)
        for (int r = 0; r < 3; ++r) c[3 * col + r] = cam->matrix[4 * col + r];
    for (int r = 0; r < 3; ++r) c[9 + r] = cam->matrix[12 + r];
    const float cam_w = 1.0f / rv::tan_det(0.5f * cam->params[1]);
    const rv::RectCamera rc = rv::rect_camera(c, cam->params[0], cam_w, width, height);
    for (size_t i = 0; i < n_tris; ++i) {
        const float *q = prepared + 16 * i;
        bool neg;
        const float a = rv::camera_numerator(rv::mk(q[0], q[1], q[2]), rv::mk(q[3], q[4], q[5]), rv::mk(c[9], c[10], c[11]), neg);
        rv::camera_rect(rc, q, q + 4, q + 8, a, rects_out[2 * i], rects_out[2 * i + 1]);
    }
    return RVPT_HIP_OK;
}

int rvpt_bounce_rows(const float *tris, const float *prepared, size_t n_tris, uint32_t *rows_out, double *scale_out)
{
    if ((n_tris && (!tris || !prepared)) || !rows_out) return RVPT_HIP_ERR_INVALID;
    if (n_tris > rv::kResidentMaxTris) return RVPT_HIP_ERR_SIZE;
    const double scale = rv::bounce_scene_scale(tris, n_tris);
    if (scale_out) *scale_out = scale;
    if (scale <= 0.0) return RVPT_HIP_OK;  // no table for this scene
    const uint32_t n = static_cast<uint32_t>(n_tris), words = (n + 31u) / 32u;
    for (uint32_t row = 0; row < 2u * n; ++row)
        for (uint32_t w = 0; w < words; ++w) rows_out[static_cast<size_t>(row) * words + w] = rv::bounce_row_word(prepared, n, row, w, rv::kBounceMarginScales * scale);
    return RVPT_HIP_OK;
}

int rvpt_claim_order(uint32_t n_work_frame, uint32_t group_blocks, uint32_t *order_out, uint32_t params_out[3])
{
    uint32_t groups = 0, stride = 1, shift = 0;
    const bool on = plan_claim_order(n_work_frame, group_blocks, groups, stride, shift);
    if (params_out) params_out[0] = on ? groups : 0u, params_out[1] = stride, params_out[2] = shift;
    if (order_out) {
        const rv::FastDiv d = rv::fast_div_make(on ? groups : 1u);
        for (uint32_t b = 0; b < n_work_frame / 64u; ++b) order_out[b] = on ? rv::claim_order_block(b, groups, stride, shift, d) : b;
    }
    return RVPT_HIP_OK;
}

int rvpt_bounce_leaf_boxes(const float *tris, size_t n_tris, float *boxes_out, uint32_t *leaf_tris_out, float *tri_boxes_out)
{
    if ((n_tris && !tris) || !boxes_out) return RVPT_HIP_ERR_INVALID;
    if (n_tris > rv::kResidentMaxTris) return RVPT_HIP_ERR_SIZE;
    if (leaf_tris_out) *leaf_tris_out = rv::kLeafTris;
    const double scale = rv::bounce_scene_scale(tris, n_tris);
    if (scale <= 0.0) return RVPT_HIP_OK;  // no table, no boxes for this scene
    rv::bounce_leaf_boxes(tris, n_tris, scale, boxes_out);
    if (tri_boxes_out) rv::bounce_group_boxes(tris, n_tris, scale, 1, tri_boxes_out);
    return RVPT_HIP_OK;
}

int rvpt_hip_selftest_camera_rects(rvpt_hip_ctx *ctx, uint32_t n_samples, uint64_t out[4], float *prepared_out, uint32_t *rects_out)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!out) return fail(ctx, RVPT_HIP_ERR_INVALID, "out is NULL");
    if (!ctx->have_scene || !ctx->have_frame) return fail(ctx, RVPT_HIP_ERR_INVALID, "selftest_camera_rects needs upload_scene and set_frame");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = sync_all(ctx)) return rc;
    std::memset(out, 0, 4 * sizeof(uint64_t));
    if (ctx->n_tris == 0) return RVPT_HIP_OK;
    rv::FrameParams p{};
    fill_frame_params(ctx, 0, p);
    uint2 *d_rects = nullptr;
    unsigned long long *d_out = nullptr;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&d_rects), ctx->n_tris * sizeof(uint2)));
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_out), 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, 4 * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) {
        const uint32_t n = static_cast<uint32_t>(ctx->n_tris);
        hipLaunchKernelGGL(rv::camera_rects, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, p, d_rects, static_cast<float4 *>(nullptr));
        hipLaunchKernelGGL(rv::selftest_camera_rects, dim3(static_cast<uint32_t>(ctx->num_cus) * 8u), dim3(256), 0, ctx->stream, p, d_rects, n_samples, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && prepared_out) e = hipMemcpyAsync(prepared_out, ctx->d_prep, ctx->n_tris * 64, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && rects_out) e = hipMemcpyAsync(rects_out, d_rects, ctx->n_tris * sizeof(uint2), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_rects);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(ctx, RVPT_HIP_ERR_HIP, "selftest_camera_rects -> %s", hipGetErrorString(e));
    return RVPT_HIP_OK;
}

int rvpt_hip_selftest_fast_div(uint32_t divisor, const uint32_t *x, uint32_t *q, size_t n)
{
    if (divisor == 0 || (n && (!x || !q))) return RVPT_HIP_ERR_INVALID;
    const rv::FastDiv f = rv::fast_div_make(divisor);
    for (size_t i = 0; i < n; ++i) q[i] = rv::fast_div(x[i], f);
    return RVPT_HIP_OK;
}

int rvpt_hip_selftest_bounce_cull(rvpt_hip_ctx *ctx, uint32_t n_samples, uint64_t out[8])
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!out) return fail(ctx, RVPT_HIP_ERR_INVALID, "out is NULL");
    if (!ctx->have_scene || !ctx->have_frame) return fail(ctx, RVPT_HIP_ERR_INVALID, "selftest_bounce_cull needs upload_scene and set_frame");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = sync_all(ctx)) return rc;
    std::memset(out, 0, 8 * sizeof(uint64_t));
    if (ctx->vis_words == 0 || ctx->n_tris == 0) return RVPT_HIP_OK;  // no table for this scene (a BVH context, too many triangles, absurd coordinates)
    rv::FrameParams p{};
    fill_frame_params(ctx, 0, p);
    p.vis = ctx->d_vis;
    p.vis_words = ctx->vis_words;
    p.vis_stride = (ctx->vis_words + 3u) & ~3u;
    p.leaf_boxes = ctx->d_leaf_boxes;
    if (ctx->have_row_boxes) p.row_bits = ctx->d_row_bits, p.row_boxes = ctx->d_row_boxes;
    unsigned long long *d_out = nullptr;
    unsigned long long h_out[6] = {};
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&d_out), 6 * sizeof(unsigned long long)));
    hipError_t e = hipMemsetAsync(d_out, 0, 6 * sizeof(unsigned long long), ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rv::selftest_bounce_cull, dim3(static_cast<uint32_t>(ctx->num_cus) * 8u), dim3(256), 0, ctx->stream, p, n_samples, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_out, d_out, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
    std::vector<uint32_t> table(static_cast<size_t>(2) * ctx->n_tris * ((ctx->vis_words + 3u) & ~3u));  // (the padding words are zero)
    if (e == hipSuccess) e = hipMemcpyAsync(table.data(), ctx->d_vis, table.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(ctx, RVPT_HIP_ERR_HIP, "selftest_bounce_cull -> %s", hipGetErrorString(e));
    out[0] = h_out[0], out[1] = h_out[1], out[4] = h_out[2], out[5] = h_out[3], out[6] = h_out[4], out[7] = h_out[5];
    for (uint32_t w : table) out[2] += static_cast<uint64_t>(__builtin_popcount(w));
    out[3] = static_cast<uint64_t>(2) * ctx->n_tris * ctx->n_tris;
    return RVPT_HIP_OK;
}

int rvpt_hip_selftest_pretest(int device_id, const float *a, const float *den, const float *closest, unsigned char *out, size_t n)
{
    if (!a || !den || !closest || !out) return fail(nullptr, RVPT_HIP_ERR_INVALID, "NULL array");
    if (n == 0) return RVPT_HIP_OK;
    if (n > (1u << 30)) return fail(nullptr, RVPT_HIP_ERR_INVALID, "n too large");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    float *d = nullptr;
    HIP_TRY(nullptr, hipMalloc(reinterpret_cast<void **>(&d), 4 * n * sizeof(float)));
    unsigned char *d_out = reinterpret_cast<unsigned char *>(d + 3 * n);
    hipError_t e = hipMemcpy(d, a, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, den, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * n, closest, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rv::selftest_camera_pretest, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, nullptr, d, d + n, d + 2 * n, d_out, static_cast<uint32_t>(n));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(nullptr, RVPT_HIP_ERR_HIP, "selftest_pretest -> %s", hipGetErrorString(e));
    return RVPT_HIP_OK;
}

int rvpt_hip_selftest_rcp(int device_id, uint64_t mismatches_per_exponent[256])
{
    if (!mismatches_per_exponent) return fail(nullptr, RVPT_HIP_ERR_INVALID, "NULL array");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    unsigned long long *d = nullptr;
    HIP_TRY(nullptr, hipMalloc(reinterpret_cast<void **>(&d), 256 * sizeof(unsigned long long)));
    hipError_t e = hipMemset(d, 0, 256 * sizeof(unsigned long long));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rv::selftest_rcp_sweep, dim3((1u << 23) / 256, 254), dim3(256), 0, nullptr, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(mismatches_per_exponent, d, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(nullptr, RVPT_HIP_ERR_HIP, "selftest_rcp -> %s", hipGetErrorString(e));
    return RVPT_HIP_OK;
}

// The stored scene as the device holds it (include/rvpt_hip_lab.h): waits like rvpt_hip_wait, then plain copies of the live bytes.  No launch, no write to
// anything the context owns.
int rvpt_hip_selftest_scene_state(rvpt_hip_ctx *ctx, rvpt_hip_scene_state_info *info, uint32_t piece, void *dst, size_t dst_capacity, size_t *bytes_out)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (bytes_out) *bytes_out = 0;
    if (!ctx->have_scene) return fail(ctx, RVPT_HIP_ERR_INVALID, "scene state before any upload_scene on this context: there is no scene to read");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (int rc = sync_all(ctx)) return rc;
    const size_t n_tris = ctx->n_tris, n_nodes = ctx->n_nodes, n_wide = ctx->n_wide;
    // the nodes the sparse update's maps cover: the end of the last level (update_geometry_sparse)
    const size_t n_map_nodes = ctx->have_sparse_maps && !ctx->refit_levels.empty() ? std::min<size_t>(n_nodes, ctx->refit_levels.back().second) : 0;
    if (info) {
        std::memset(info, 0, sizeof *info);
        info->n_tris = n_tris, info->n_nodes = n_nodes, info->n_wide = n_wide;
        info->bvh_head_shift = ctx->bvh_head_shift, info->wide_stack_levels = ctx->wide_stack_levels, info->bvh_height = ctx->bvh_height;
        info->built_by = static_cast<uint32_t>(ctx->built_by);
        info->have_perm = ctx->have_perm, info->have_sparse_maps = ctx->have_sparse_maps, info->have_inv_perm = ctx->have_inv_perm, info->have_cost = ctx->have_cost;
        info->base_cost = ctx->base_cost;
    }
    const void *src = nullptr;
    bool host = false;
    size_t bytes = 0;
    switch (piece) {
    case RVPT_HIP_STATE_NONE: break;
    case RVPT_HIP_STATE_NODES: src = ctx->d_nodes, bytes = n_nodes * sizeof(rvpt_bvh_node); break;
    case RVPT_HIP_STATE_TRIS: src = ctx->d_tris, bytes = n_tris * sizeof(rvpt_triangle); break;
    case RVPT_HIP_STATE_PERM: src = ctx->d_perm, bytes = ctx->have_perm ? n_tris * sizeof(uint32_t) : 0; break;
    case RVPT_HIP_STATE_WIDE: src = ctx->d_wide, bytes = n_wide * 128u; break;
    case RVPT_HIP_STATE_WIDE_MAP: src = ctx->d_wide_map, bytes = n_wide * 16u; break;
    case RVPT_HIP_STATE_REFIT_LEVELS: src = ctx->refit_levels.data(), bytes = ctx->refit_levels.size() * 2u * sizeof(uint32_t), host = true; break;
    case RVPT_HIP_STATE_SPARSE_PARENT: src = ctx->d_sparse_parent, bytes = n_map_nodes * sizeof(uint32_t); break;
    case RVPT_HIP_STATE_SPARSE_LEAF_OF: src = ctx->d_sparse_leaf_of, bytes = n_map_nodes ? n_tris * sizeof(uint32_t) : 0; break;
    case RVPT_HIP_STATE_SPARSE_DIRTY: src = ctx->d_sparse_dirty, bytes = n_map_nodes * sizeof(uint32_t); break;
    case RVPT_HIP_STATE_INV_PERM: src = ctx->d_inv_perm, bytes = ctx->have_perm && ctx->have_inv_perm ? n_tris * sizeof(uint32_t) : 0; break;
    case RVPT_HIP_STATE_REST:  // the pose update's rest pose: on the device of a BVH context, on the host of a brute-force one
        if (is_bvh(ctx, n_tris)) src = ctx->d_rest;
        else src = ctx->h_rest.data(), host = true;
        bytes = ctx->have_rest ? n_tris * offsetof(rvpt_triangle, mat_id) : 0;
        break;
    case RVPT_HIP_STATE_SKIN:  // the binding, in the update form's order: on the device of a BVH context, on the host of a brute-force one
        if (is_bvh(ctx, n_tris)) src = ctx->d_skin;
        else src = ctx->h_skin.data(), host = true;
        bytes = ctx->have_skin ? 3 * n_tris * sizeof(rvpt_vertex_skin) : 0;
        break;
    case RVPT_HIP_STATE_BONES: src = ctx->d_bones, bytes = ctx->have_skin ? ctx->skin_bones * sizeof(rvpt_bone) : 0; break;
    default: return fail(ctx, RVPT_HIP_ERR_INVALID, "scene state: there is no piece %u", piece);
    }
    if (bytes_out) *bytes_out = bytes;
    if (bytes == 0) return RVPT_HIP_OK;
    if (!src) return fail(ctx, RVPT_HIP_ERR_INVALID, "scene state: piece %u has %zu live bytes and no buffer", piece, bytes);
    if (!dst || dst_capacity < bytes) return fail(ctx, RVPT_HIP_ERR_SIZE, "scene state: piece %u needs %zu bytes, dst holds %zu", piece, bytes, dst ? dst_capacity : size_t(0));
    if (host) std::memcpy(dst, src, bytes);
    else HIP_TRY(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RVPT_HIP_OK;
}

#endif  // RVPT_HIP_LAB

int rvpt_hip_untile(rvpt_hip_ctx *ctx, const void *gathered_dev, size_t slot_bytes, uint32_t n_ranks, void *dst_dev_rgba32f)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!gathered_dev || !dst_dev_rgba32f || n_ranks == 0 || slot_bytes % sizeof(float4)) return fail(ctx, RVPT_HIP_ERR_INVALID, "bad untile arguments");
    const size_t need = static_cast<size_t>(owned_tiles(ctx->tiles_x * ctx->tiles_y, 0, n_ranks)) * 256u * sizeof(float4);
    if (slot_bytes < need) return fail(ctx, RVPT_HIP_ERR_SIZE, "slot holds %zu bytes, rank 0 of %u needs %zu", slot_bytes, n_ranks, need);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const dim3 blk(64, 4), grd((ctx->width + 63) / 64, (ctx->height + 3) / 4);
    hipLaunchKernelGGL(rv::untile_rgba32f, grd, blk, 0, ctx->stream, static_cast<const float4 *>(gathered_dev), slot_bytes / sizeof(float4),
                       n_ranks, ctx->width, ctx->height, ctx->tiles_x, static_cast<float4 *>(dst_dev_rgba32f));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RVPT_HIP_OK;
}

int rvpt_hip_write_accum(rvpt_hip_ctx *ctx, const void *src_rgba32f, size_t src_bytes)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    const size_t need = static_cast<size_t>(ctx->width) * ctx->height * 16;
    if (!src_rgba32f) return fail(ctx, RVPT_HIP_ERR_INVALID, "src is NULL");
    if (src_bytes < need) return fail(ctx, RVPT_HIP_ERR_SIZE, "src holds %zu bytes, frame needs %zu", src_bytes, need);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool device_src = false;
    int rc = classify_frame_pointer(ctx, src_rgba32f, "src", &device_src);
    if (rc) return rc;
    if (device_src) {  // tiled straight from the caller's device memory (whatever wrote it has finished: the caller's word); no staging buffer
        if (ctx->n_work) {
            if (reinterpret_cast<uintptr_t>(src_rgba32f) % 16u == 0)
                hipLaunchKernelGGL(rv::tile_rgba32f, dim3((ctx->n_work + 255) / 256), dim3(256), 0, ctx->stream, static_cast<const float4 *>(src_rgba32f), ctx->width, ctx->height,
                                   ctx->tiles_x, ctx->tile_rank, ctx->tile_world, ctx->n_work, ctx->d_accum);
            else  // (tile_rgba32f loads a pixel as one float4)
                hipLaunchKernelGGL(rv::tile_rgba32f_dwords, dim3((ctx->n_work + 63) / 64), dim3(256), 0, ctx->stream, static_cast<const float *>(src_rgba32f), ctx->width, ctx->height,
                                   ctx->tiles_x, ctx->tile_rank, ctx->tile_world, ctx->n_work, reinterpret_cast<float *>(ctx->d_accum));
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return RVPT_HIP_OK;
    }
    if ((rc = ensure_rowmajor(ctx))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_rowmajor, src_rgba32f, need, hipMemcpyHostToDevice, ctx->stream));
    if (ctx->n_work) {
        hipLaunchKernelGGL(rv::tile_rgba32f, dim3((ctx->n_work + 255) / 256), dim3(256), 0, ctx->stream, static_cast<const float4 *>(ctx->d_rowmajor),
                           ctx->width, ctx->height, ctx->tiles_x, ctx->tile_rank, ctx->tile_world, ctx->n_work, ctx->d_accum);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RVPT_HIP_OK;
}

int rvpt_hip_get_timing(rvpt_hip_ctx *ctx, float *kernel_ms_last, double *kernel_ms_sum, uint64_t *n_dispatches)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!ctx->timing) return fail(ctx, RVPT_HIP_ERR_INVALID, "context created without RVPT_HIP_TIMING");
    int rc = drain_timing(ctx);
    if (rc) return rc;
    if (kernel_ms_last) *kernel_ms_last = ctx->last_ms;
    if (kernel_ms_sum) *kernel_ms_sum = ctx->sum_ms;
    if (n_dispatches) *n_dispatches = ctx->n_timed;
    return RVPT_HIP_OK;
}

int rvpt_hip_reset_timing(rvpt_hip_ctx *ctx)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->timing) {
        int rc = drain_timing(ctx);
        if (rc) return rc;
    }
    ctx->last_ms = 0.f;
    ctx->sum_ms = 0.0;
    ctx->n_timed = 0;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_stats, 0, rv::kStatStripes * rv::kStatStride * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RVPT_HIP_OK;
}

int rvpt_hip_get_stats(rvpt_hip_ctx *ctx, uint64_t stats[2])
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!stats) return fail(ctx, RVPT_HIP_ERR_INVALID, "stats is NULL");
    if (!(ctx->flags & RVPT_HIP_COUNT_SEGMENTS)) return fail(ctx, RVPT_HIP_ERR_INVALID, "context created without RVPT_HIP_COUNT_SEGMENTS");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long h[rv::kStatStripes * rv::kStatStride] = {};  // (64 pairs, one cache line each: rvpt_kernels.h)
    HIP_TRY(ctx, hipMemcpyAsync(h, ctx->d_stats, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    stats[0] = stats[1] = 0;
    for (uint32_t s = 0; s < rv::kStatStripes; ++s) {
        stats[0] += h[rv::kStatStride * s + 0];
        stats[1] += h[rv::kStatStride * s + 1];
    }
    return RVPT_HIP_OK;
}

int rvpt_hip_get_launch_info(rvpt_hip_ctx *ctx, uint32_t *grid_blocks, uint32_t *lds_bytes, uint32_t *kernel_variant,
                             uint32_t *frames_in_flight)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (ctx->last_grid == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "no frame dispatched yet");
    if (grid_blocks) *grid_blocks = ctx->last_grid;
    if (lds_bytes) *lds_bytes = ctx->last_lds;
    if (kernel_variant) *kernel_variant = ctx->last_variant;
    if (frames_in_flight) *frames_in_flight = static_cast<uint32_t>(ctx->last_slots ? ctx->last_slots : slots_for(ctx, 1));
    return RVPT_HIP_OK;
}

int rvpt_hip_get_cull_info(rvpt_hip_ctx *ctx, uint32_t *flags)
{
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    if (!flags) return fail(ctx, RVPT_HIP_ERR_INVALID, "flags is NULL");
    if (ctx->last_grid == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "no frame dispatched yet");
    *flags = ctx->last_cull;
    return RVPT_HIP_OK;
}

const char *rvpt_hip_last_error(rvpt_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

}  // extern "C"
