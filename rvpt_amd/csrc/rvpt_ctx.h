// rvpt_ctx.h — the context behind the C ABI of include/rvpt_hip.h and the few helpers every host file of the library uses.  Internal: rvpt_abi.hip (create /
// destroy, launch planning, dispatch, collectives, reads) and rvpt_scene.hip (every form of rvpt_hip_upload_scene) include it; nothing here has C linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rvpt_hip.h"
#include "rvpt_kernels.h"

#ifndef RVPT_HIP_LAB
#define RVPT_HIP_LAB 0  // 1: the laboratory build (librvpt_hip_debug.so): + the selftests and host-side forms of include/rvpt_hip_lab.h, the opt-in walks, the tuning knobs
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
    // the BUILD FORM of upload_scene (rvpt_build.h; rvpt_scene.hip: build_scene_on_device): the permutation it sorted the caller's triangles by (perm[j] = caller's index of
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
    float4 *d_row_caps = nullptr;             // ... and every row's cap (rvpt_vis.h: the row caps), one float4 per row, made behind the row boxes
    size_t row_caps_cap = 0;                  // in float4
    bool row_caps_on = false;                 // ... with finite caps (the laboratory build's RVPT_HIP_PACKETS_ROW_CAPS=0: every K = +inf, no round skips)
    bool have_row_boxes = false;              // made for the scene in d_prep (row boxes and row caps)
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

// ---- the helpers every host file uses (defined once, in rvpt_abi.hip; hidden: the library exports the C ABI and nothing else) -------------------------------

#define RVPT_INTERNAL __attribute__((visibility("hidden")))

// the message behind a return code: into ctx->err, or, before a context exists (ctx == NULL), into the thread's own string; returns `code`
RVPT_INTERNAL int fail(rvpt_hip_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(ctx, RVPT_HIP_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
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

// every frame kernel in flight, then everything queued behind them on the main stream
RVPT_INTERNAL int sync_all(rvpt_hip_ctx *ctx);

// a BVH context with triangles, hence a tree (upload_scene); an empty scene's frames run the brute-force instances over zero triangles
inline bool is_bvh(const rvpt_hip_ctx *ctx, size_t n_tris) { return (ctx->flags & RVPT_HIP_TRAVERSAL_MASK) != RVPT_HIP_TRAVERSAL_BRUTE && n_tris > 0; }

// the GPU whose memory `p` is (hipMalloc: a torch tensor's storage, say), -1: host memory.  Pinned and managed memory can be read on the host and count as
// host memory.
RVPT_INTERNAL int device_of_pointer(const void *p);
inline bool is_device_pointer(const void *p) { return device_of_pointer(p) >= 0; }
