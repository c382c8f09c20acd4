// rvpt_abi.hip — implementation of the C ABI declared in include/rvpt_hip.h.
//
// Host-side counterpart of the reference seam inside `class RVPT` (src/rvpt/rvpt.cpp): resource
// creation (:639-866), per-frame upload (:96-126), dispatch (:1005-1039, :352-354) and the fence
// (:115-116) become HIP runtime calls on one stream of one device.  No exception leaves this file.
// Here: create / destroy, launch planning, dispatch, the collectives, the read formats and the laboratory entry points.  The context itself is rvpt_ctx.h's;
// rvpt_hip_upload_scene, in all its forms, is rvpt_scene.hip's.
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
#include "rvpt_ctx.h"
#include "rvpt_kernels.h"
#include "bvh_wide.h"
#include "rvpt_refit.h"
#include "rvpt_frames.h"
#include "rvpt_build.h"
#include "rvpt_query.h"
#include "rvpt_nearest.h"
#include "rvpt_box.h"
#include "rvpt_sweep.h"
#include "rvpt_surface.h"
#include "rvpt_paths.h"
#include "rvpt_packets.h"
#include "rvpt_math.h"
#include "rvpt_rect.h"
#include "rvpt_vis.h"

#ifndef RV_REPORT_STACK_OVERFLOW
#define RV_REPORT_STACK_OVERFLOW 0  // (rvpt_device.h) 1: the BVH kernels report a push past the stack the host sized
#endif

static_assert(rv::kWideChildren == rv::kWideFormChildren && rv::kWideEmpty == rv::kWideFormEmpty, "bvh_wide.h and rvpt_kernels.h describe the same node");
static_assert(sizeof(rvpt_triangle) == 64, "Triangle layout (structs.glsl:1-7)");
static_assert(sizeof(rvpt_bvh_node) == 32, "BvhNode layout (structs.glsl:9-14)");
static_assert(sizeof(rvpt_material) == 48, "Material layout (structs.glsl:22-33)");
static_assert(sizeof(rvpt_render_settings) == 40, "RenderSettings std140 block (compute_pass.comp:28-40)");
static_assert(sizeof(rvpt_camera_data) == 80, "Camera block (compute_pass.comp:44-49)");
static_assert(RVPT_HIP_RAY_MAX_HITS == rv::kQueryMaxHits, "the k of a k-nearest ray query: the header's and the kernels'");
static_assert(RVPT_HIP_POINT_MAX_NEAREST == rv::kNearestMaxK, "the k of a k-nearest point query: the header's and the kernels'");
static_assert(RVPT_HIP_BOX_MAX_GROUP == rv::kBoxMaxGroup, "the k of a box query's group: the header's and the kernels'");
static_assert(sizeof(rvpt_box_overlap) == rv::kBoxRecordBytes && offsetof(rvpt_box_overlap, prim_from) == 12 && offsetof(rvpt_box_overlap, hi) == 16 &&
                  offsetof(rvpt_box_overlap, flags) == 28 && offsetof(rvpt_box_overlap, count) == 32 && offsetof(rvpt_box_overlap, prim) == 36,
              "a box query's record: three float4 (rvpt_box.hip)");
static_assert(sizeof(rvpt_sphere_sweep) == rv::kSweepRecordBytes && sizeof(rvpt_sphere_sweep) == sizeof(rvpt_ray_hit) && offsetof(rvpt_sphere_sweep, radius) == 12 &&
                  offsetof(rvpt_sphere_sweep, dir) == 16 && offsetof(rvpt_sphere_sweep, tmax) == 28 && offsetof(rvpt_sphere_sweep, t) == 32 && offsetof(rvpt_sphere_sweep, prim) == 36 &&
                  offsetof(rvpt_sphere_sweep, u) == 40 && offsetof(rvpt_sphere_sweep, v) == 44,
              "a sphere sweep's record: three float4 (rvpt_sweep.hip), its out quad laid out as a ray record's, and it shares query_records");
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

// NOTE: the library does not touch the process environment.  Frames in flight want GPU_MAX_HW_QUEUES >= 8 set by the
// HOST before HIP initialises (include/rvpt_hip.h); rvpt_render, the Python package and bench.py do so.

namespace {
thread_local std::string g_err;  // for calls that fail before a context exists
}

// The helpers rvpt_ctx.h declares for every file of the library, defined here once.
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

// every frame kernel in flight, then everything queued behind them on the main stream
int sync_all(rvpt_hip_ctx *ctx)
{
    for (int i = 0; i < ctx->n_slots; ++i) HIP_TRY(ctx, hipStreamSynchronize(ctx->trace_stream[i]));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Plain host memory is unknown to the runtime, which answers with an error and keeps it as the thread's last error: cleared here.
int device_of_pointer(const void *p)
{
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return attr.type == hipMemoryTypeDevice ? attr.device : -1;
}

namespace {

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

#define RCCL_TRY(ctx, expr)                                                                                       \
    do {                                                                                                          \
        ncclResult_t r_ = (expr);                                                                                 \
        if (r_ != ncclSuccess) return fail(ctx, RVPT_HIP_ERR_COMM, "%s -> %s", #expr, rccl().GetErrorString(r_)); \
    } while (0)

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
constexpr uint32_t kCullRowCaps = 2048u;  // ... and with finite row caps: uniform rounds whose rays all rise above their row's cap walk nothing (rvpt_vis.h: the row caps)
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
            if (p.leaf_boxes && k.packets_row_boxes && ctx->have_row_boxes) p.row_bits = ctx->d_row_bits, p.row_boxes = ctx->d_row_boxes, p.row_caps = ctx->d_row_caps;
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
                  ((p.row_boxes && ctx->row_rule_tight) ? kCullRowRuleTight : 0u) | ((p.row_boxes && ctx->row_caps_on) ? kCullRowCaps : 0u);
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
    if (ctx->d_row_caps) (void)hipFree(ctx->d_row_caps);
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

// The frame pointer of rvpt_hip_read / rvpt_hip_write_accum (`what`: "dst" / "src"): host memory, or device memory of the context's GPU, which the layout kernels
// then write or read in place.  Device memory of another GPU and device memory that is not 4-byte aligned are refused before anything touches them.
static int classify_frame_pointer(rvpt_hip_ctx *ctx, const void *p, const char *what, bool *device)
{
    const int dev = device_of_pointer(p);
    *device = dev >= 0;
    if (!*device) return RVPT_HIP_OK;
    if (dev != ctx->device)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "%s is device memory of GPU %d, the context lives on GPU %d: a frame stays on the context's own device", what, dev, ctx->device);
    if (reinterpret_cast<uintptr_t>(p) % 4u)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "%s is device memory at %p: a frame on the device needs 4-byte alignment", what, p);
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
// per record as before.  (RecordKind::Points: 0 for RVPT_HIP_FORMAT_NEAREST_POINTS and RVPT_HIP_FORMAT_NEAREST_POINTS_K(1), the same call; k for
// RVPT_HIP_FORMAT_NEAREST_POINTS_K(k), k > 1 (K-NEAREST POINTS) — groups of k records, one point each, likewise.)
// RecordKind::Crossings (RVPT_HIP_FORMAT_RAY_CROSSINGS, RAY CROSSINGS): a ray query in everything but the kernels and the record's name.
// RecordKind::Boxes (RVPT_HIP_FORMAT_BOX_OVERLAPS, BOX OVERLAPS): a point query's scene under the kernels of rvpt_box.hip; `hits` is 0 for format 9 and for
// RVPT_HIP_FORMAT_BOX_OVERLAPS_K(1), the same call, and k for RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k), k > 1 — groups of k records, one box each; only the third quad
// of a record is out.
// RecordKind::Sweeps (RVPT_HIP_FORMAT_SPHERE_SWEEPS, SPHERE SWEEPS): a point query's scene under the kernels of rvpt_sweep.hip; the third quad of a record is out.
enum class RecordKind { Rays, Paths, Points, Surface, Crossings, Boxes, Sweeps };
static int query_records(rvpt_hip_ctx *ctx, void *dst, size_t dst_bytes, const RecordKind kind, const uint32_t path_mode = rv::kPathModeKajiya, const uint32_t hits = 0)
{
    const bool paths = kind == RecordKind::Paths, points = kind == RecordKind::Points, surface = kind == RecordKind::Surface, crossings = kind == RecordKind::Crossings;
    const bool boxes = kind == RecordKind::Boxes, sweeps = kind == RecordKind::Sweeps;
    const char *what = sweeps ? "sweep" : boxes ? "box" : surface ? "surface" : (points ? "point" : (paths ? "path" : (crossings ? "crossing" : "ray")));
    const char *record = sweeps ? "rvpt_sphere_sweep" : boxes ? "rvpt_box_overlap" : surface ? "rvpt_surface_point" : (points ? "rvpt_point_hit" : (paths ? "rvpt_ray_path" : (crossings ? "rvpt_ray_crossings" : "rvpt_ray_hit")));
    static_assert(sizeof(rvpt_ray_crossings) == sizeof(rvpt_ray_hit) && offsetof(rvpt_ray_crossings, front) == offsetof(rvpt_ray_hit, t), "a crossing record is laid out as a ray record");
    const size_t out_offset = surface ? offsetof(rvpt_surface_point, point) : (points ? offsetof(rvpt_point_hit, closest) : offsetof(rvpt_ray_hit, t));  // where a record's out fields begin
    if (hits && boxes && dst_bytes % (sizeof(rvpt_box_overlap) * hits))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "box query with k = %u: dst_bytes %zu is not a multiple of the %zu bytes of a group of k rvpt_box_overlap", hits, dst_bytes,
                    sizeof(rvpt_box_overlap) * hits);
    if (hits && points && dst_bytes % (sizeof(rvpt_point_hit) * hits))
        return fail(ctx, RVPT_HIP_ERR_INVALID, "point query with k = %u: dst_bytes %zu is not a multiple of the %zu bytes of a group of k rvpt_point_hit", hits, dst_bytes,
                    sizeof(rvpt_point_hit) * hits);
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
    scene.unit_n = ctx->d_unit_n;
    scene.n_tris = static_cast<uint32_t>(ctx->n_tris), scene.n_wide = static_cast<uint32_t>(ctx->n_wide), scene.head_shift = ctx->bvh_head_shift;
    scene.stack_levels = scene.kind == rv::QueryKind::Wide ? ctx->wide_stack_levels : bvh_stack_levels(ctx);
    path_scene.mat_index = ctx->d_mat_index, path_scene.unit_n = ctx->d_unit_n, path_scene.mats = ctx->d_mats;
    rv::NearestScene nearest{};  // a point query reads the vertex rows and the binary nodes, whichever form the ray walks of this context take
    nearest.brute = !bvh;
    nearest.tris = ctx->d_tris, nearest.nodes = ctx->d_nodes, nearest.perm = scene.perm;
    nearest.n_tris = scene.n_tris, nearest.n_nodes = static_cast<uint32_t>(ctx->n_nodes), nearest.stack_levels = bvh_stack_levels(ctx);
    const uint32_t groups_of = hits ? hits : 1u;  // records per ray, per point or per box
    const rv::QueryForm ray_form = crossings ? rv::QueryForm::Crossings : rv::QueryForm::Hits;
    rv::QueryPlan plan{};
    if (sweeps)
        HIP_TRY(ctx, rv::sweep_plan(nearest, static_cast<uint32_t>(n), ctx->num_cus, &plan));
    else if (boxes)
        HIP_TRY(ctx, rv::box_plan(nearest, static_cast<uint32_t>(n / groups_of), ctx->num_cus, &plan, groups_of));
    else if (points)
        HIP_TRY(ctx, rv::nearest_plan(nearest, static_cast<uint32_t>(n / groups_of), ctx->num_cus, &plan, groups_of));
    else if (paths)
        HIP_TRY(ctx, rv::path_plan(path_scene, static_cast<uint32_t>(n), ctx->num_cus, path_mode, &plan));
    else if (!surface)  // (a surface read is one record per lane and no walk: no plan, no stack)
        HIP_TRY(ctx, rv::query_plan(scene, ray_form, static_cast<uint32_t>(n / groups_of), ctx->num_cus, &plan, groups_of));
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
    } else if (sweeps)
        HIP_TRY(ctx, rv::sweep_launch(ctx->stream, nearest, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n)));
    else if (boxes)
        HIP_TRY(ctx, rv::box_launch(ctx->stream, nearest, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n / groups_of), groups_of));
    else if (points)
        HIP_TRY(ctx, rv::nearest_launch(ctx->stream, nearest, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n / groups_of), groups_of));
    else if (paths)
        HIP_TRY(ctx, rv::path_launch(ctx->stream, path_scene, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n), path_mode));
    else
        HIP_TRY(ctx, rv::query_launch(ctx->stream, scene, ray_form, plan, ctx->d_query_scratch, records, static_cast<uint32_t>(n / groups_of), groups_of));
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
    if (format == RVPT_HIP_FORMAT_NEAREST_POINTS_K(1)) return query_records(ctx, dst, dst_bytes, RecordKind::Points);  // k = 1 IS format 4, its messages included
    if (format > RVPT_HIP_FORMAT_NEAREST_POINTS_K(1) && format <= static_cast<int>(RVPT_HIP_FORMAT_NEAREST_POINTS_K(RVPT_HIP_POINT_MAX_NEAREST)))  // the k nearest triangles of a point; local as well
        return query_records(ctx, dst, dst_bytes, RecordKind::Points, rv::kPathModeKajiya, static_cast<uint32_t>(format) - RVPT_HIP_FORMAT_NEAREST_POINTS_K(0u));
    if (format == RVPT_HIP_FORMAT_TRIANGLES) return read_triangles(ctx, dst, dst_bytes);  // local as well
    if (format == RVPT_HIP_FORMAT_SURFACE_POINTS) return query_records(ctx, dst, dst_bytes, RecordKind::Surface);
    if (format == RVPT_HIP_FORMAT_RAY_CROSSINGS) return query_records(ctx, dst, dst_bytes, RecordKind::Crossings);  // local as well
    if (format == RVPT_HIP_FORMAT_BOX_OVERLAPS || format == RVPT_HIP_FORMAT_BOX_OVERLAPS_K(1)) return query_records(ctx, dst, dst_bytes, RecordKind::Boxes);  // k = 1 IS format 9, its messages included; local as well
    if (format > RVPT_HIP_FORMAT_BOX_OVERLAPS_K(1) && format <= static_cast<int>(RVPT_HIP_FORMAT_BOX_OVERLAPS_K(RVPT_HIP_BOX_MAX_GROUP)))  // the longer lists of a box query; local as well
        return query_records(ctx, dst, dst_bytes, RecordKind::Boxes, rv::kPathModeKajiya, static_cast<uint32_t>(format) - RVPT_HIP_FORMAT_BOX_OVERLAPS_K(0u));
    if (format == RVPT_HIP_FORMAT_SPHERE_SWEEPS) return query_records(ctx, dst, dst_bytes, RecordKind::Sweeps);  // local as well
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
    if (ctx->have_row_boxes) p.row_bits = ctx->d_row_bits, p.row_boxes = ctx->d_row_boxes, p.row_caps = ctx->d_row_caps;
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
