// rvpt_scene.hip — rvpt_hip_upload_scene (include/rvpt_hip.h) in all its forms: the full upload, the three device builds, the plain, guarded and sparse updates,
// the pose and skin updates with their guarded forms, and the bind.  Host code only: the kernels it launches live in rvpt_kernels.hip, rvpt_packets.hip,
// rvpt_refit.hip and the three build files.  Which form a call is, and what a form does to the rest pose and the binding afterwards, is rvpt_scene_forms.h's;
// the entry point at the end of this file classifies, switches to the form and applies that table.  No exception leaves this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "rvpt_ctx.h"
#include "rvpt_scene_forms.h"
#include "rvpt_kernels.h"
#include "rvpt_packets.h"
#include "bvh_wide.h"
#include "rvpt_refit.h"
#include "rvpt_build.h"
#include "rvpt_vis.h"

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
            // ... and the row caps behind them (rvpt_vis.h), from the records and the hit normals
            if ((rc = grow(ctx, ctx->d_row_caps, ctx->row_caps_cap, static_cast<size_t>(2) * n, sizeof(float4)))) return rc;
            bool caps = true;
#if RVPT_HIP_LAB
            if (const char *e = getenv("RVPT_HIP_PACKETS_ROW_CAPS")) caps = atoi(e) > 0;  // read at every upload: 0 = every cap +inf, no round skips (A/B, bit-exactness)
#endif
            hipLaunchKernelGGL(rv::bounce_row_caps, dim3((2u * n + 63u) / 64u), dim3(64), 0, ctx->stream, ctx->d_prep, ctx->d_unit_n, n, scale, words, caps ? 1u : 0u, ctx->d_row_caps);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->have_row_boxes = true;
            ctx->row_rule_tight = tight;
            ctx->row_caps_on = caps;
        }
    }
    return 0;
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

// Every update form of a BVH context walks the level table of the breadth-first device layout.  (It is missing under the laboratory's knob only: the release
// library always makes that layout and names no laboratory knob.)
static int require_level_table(rvpt_hip_ctx *ctx, bool bvh)
{
    if (!bvh || !ctx->refit_levels.empty()) return RVPT_HIP_OK;
#if RVPT_HIP_LAB
    return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the breadth-first device layout of the tree: RVPT_HIP_BVH_CALLER_LAYOUT keeps the caller's, which has no level ranges");
#else
    return fail(ctx, RVPT_HIP_ERR_UNSUPPORTED, "geometry update needs the level ranges of the tree's device layout, which this context does not hold");
#endif
}

static int update_geometry(rvpt_hip_ctx *ctx, const rvpt_triangle *tris, size_t n_tris)
{
    if (!ctx->have_scene)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "geometry update (no nodes, no materials) before any full upload_scene on this context: there is no scene to update");
    if (n_tris != ctx->n_tris)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "geometry update with %zu triangles, the uploaded scene has %zu: a full upload_scene changes the count", n_tris, ctx->n_tris);
    const bool bvh = is_bvh(ctx, n_tris);
    if (int rc0 = require_level_table(ctx, bvh)) return rc0;
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
    if (int rc0 = require_level_table(ctx, bvh)) return rc0;
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

// The REST POSE, shared by the pose and the skin forms (rvpt_hip_ctx::have_rest).  BVH contexts: the snapshot if the context holds none for the stored scene —
// 48 of every 64 bytes of d_tris, device to device, in stored order, on ctx->stream.
static int ensure_rest_snapshot(rvpt_hip_ctx *ctx)
{
    if (ctx->have_rest) return RVPT_HIP_OK;
    const size_t n_tris = ctx->n_tris;
    if (int rc = grow(ctx, ctx->d_rest, ctx->cap_rest, 3 * n_tris, sizeof(float4))) return rc;
    HIP_TRY(ctx, hipMemcpy2DAsync(ctx->d_rest, offsetof(rvpt_triangle, mat_id), ctx->d_tris, sizeof(rvpt_triangle), offsetof(rvpt_triangle, mat_id), n_tris, hipMemcpyDeviceToDevice,
                                  ctx->stream));
    ctx->have_rest = true;
    return RVPT_HIP_OK;
}

// Brute-force contexts keep the rest pose on the host: the stored records are read back, snapshotted if the context holds no rest pose, moved by the form, and
// go through the plain update form.  `move_triangles(pose_rows)` names the triangles its form moves: it calls pose_rows(t, vertex) for each, and
// vertex(v, p, out) is the form's arithmetic for vertex v of that triangle at the rest position p.  The w lanes come from the rest pose.
template <typename MoveTriangles>
static int update_from_host_rest(rvpt_hip_ctx *ctx, MoveTriangles move_triangles)
{
    const size_t n_tris = ctx->n_tris;
    if (int rc0 = sync_all(ctx)) return rc0;
    std::vector<rvpt_triangle> posed(n_tris);
    HIP_TRY(ctx, hipMemcpy(posed.data(), ctx->d_tris, n_tris * sizeof(rvpt_triangle), hipMemcpyDeviceToHost));
    if (!ctx->have_rest) {
        ctx->h_rest.resize(12 * n_tris);
        for (size_t t = 0; t < n_tris; ++t) std::memcpy(&ctx->h_rest[12 * t], &posed[t], offsetof(rvpt_triangle, mat_id));
        ctx->have_rest = true;
    }
    move_triangles([&](size_t t, auto vertex) {
        const float *r = &ctx->h_rest[12 * t];
        float *rows[3] = {posed[t].vert0, posed[t].vert1, posed[t].vert2};
        for (int v = 0; v < 3; ++v) {
            vertex(v, r + 4 * v, rows[v]);
            rows[v][3] = r[4 * v + 3];
        }
    });
    const int rc0 = update_geometry(ctx, posed.data(), n_tris);
    if (rc0 == RVPT_HIP_OK) ctx->err.clear();
    return rc0;
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
    if (int rc0 = require_level_table(ctx, bvh)) return rc0;
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

    if (!bvh)  // the rest pose on the host, the listed ranges posed there
        return update_from_host_rest(ctx, [&](auto pose_rows) {
            for (size_t p = 0; p < k; ++p)
                for (size_t t = moves[p].first; t < static_cast<size_t>(moves[p].first) + moves[p].count; ++t)
                    pose_rows(t, [&](int, const float *r, float *out) { pose_vertex_host(moves[p].m, r, out); });
        });

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
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight finish on the old geometry
    if ((rc = ensure_rest_snapshot(ctx))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sparse_stage, moves, k * sizeof(rvpt_part_move), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_sparse_stage + k * sizeof(rvpt_part_move), prefix.data(), (k + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
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
    if (int rc0 = require_level_table(ctx, bvh)) return rc0;
    list->dev = dev, list->bvh = bvh;
    return RVPT_HIP_OK;
}

static int skin_execute(rvpt_hip_ctx *ctx, const rvpt_bone *bones, size_t k, const SkinList &list)
{
    const size_t n_tris = ctx->n_tris;
    const int dev = list.dev;
    const bool bvh = list.bvh;

    if (!bvh)  // the rest pose on the host, every triangle skinned there
        return update_from_host_rest(ctx, [&](auto pose_rows) {
            for (size_t t = 0; t < n_tris; ++t)
                pose_rows(t, [&](int v, const float *r, float *out) { skin_vertex_host(bones, ctx->h_skin[3 * t + v], r, out); });
        });

    int rc;
    const uint32_t n = static_cast<uint32_t>(n_tris), kk = static_cast<uint32_t>(k);
    if ((rc = grow(ctx, ctx->d_bones, ctx->cap_bones, 3 * static_cast<size_t>(RVPT_HIP_SKIN_MAX_BONES), sizeof(float4)))) return rc;
    if (int rc0 = sync_all(ctx)) return rc0;  // frames in flight finish on the old geometry
    if ((rc = ensure_rest_snapshot(ctx))) return rc;
    ctx->skin_bones = 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bones, bones, k * sizeof(rvpt_bone), dev >= 0 ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
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

// THE GUARD of the guarded update, the guarded pose update and the guarded skin update (include/rvpt_hip.h), in three pieces: the one refusal of a guarded
// form, the tail behind its update, and the order the two take around a form that comes in two halves.
//
// The refusal: a limit on a tree that came from an ordinary upload — the library has no builder to rebuild it by.  Report only (0) is legal there.
// (Spelled out per form: tests/test_scene_model_host.py looks for these sentences in this file's text.)
static int refuse_limit_without_builder(rvpt_hip_ctx *ctx, const rv::SceneCall &call)
{
    if (call.permille == 0 || ctx->built_by != rvpt_hip_ctx::kBuiltByCaller) return RVPT_HIP_OK;
    switch (call.form) {
    case rv::SceneForm::PoseGuarded:
        return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded pose update with a limit after an ordinary upload_scene: the tree is the caller's, the library has no builder to rebuild it by (report only, limit 0, is legal)");
    case rv::SceneForm::SkinGuarded:
        return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded skin update with a limit after an ordinary upload_scene: the tree is the caller's, the library has no builder to rebuild it by (report only, limit 0, is legal)");
    default:
        return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded update with a limit after an ordinary upload_scene: the tree is the caller's, the library has no builder to rebuild it by (report only, limit 0, is legal)");
    }
}

// The tail, behind the form's update: the cost of the stored tree — boxes the update left alone enter it as they are, loose ones included —, the decision, and
// either the report "refitted" or, with a limit, once the cost has grown past limit x base cost, the rebuild by the builder that made the stored tree and the
// report "rebuilt".  The rebuild: d_tris (moved vertices beside the stored mat_id rows, leaf order) into d_carry in the caller's order by the old permutation —
// a buffer of its own: the build reads its source until its last gather and writes d_tris, d_prep and its scratch meanwhile — and, where the form's row says
// so, the rest pose beside it into d_rest_carry, and behind the build back into stored order by the new permutation, so that the next pose or skin update
// poses from the same rest pose as before.  d_skin is not touched: it is in the caller's order and is read through d_perm.  permille: 0 (report only) or
// 1000 .. 65535, checked by the caller.
static int guarded_tail(rvpt_hip_ctx *ctx, const rv::SceneFormRow &row, uint32_t permille)
{
    double cost = 0.0;
    bool have = false;
    if (int rc = device_tree_cost(ctx, &cost, &have)) return rc;
    const double base = ctx->base_cost;
    // (have_perm: the pose and skin forms asked for it, the plain form did not.  It cannot matter there: with a limit this line is reached only past
    // refuse_limit_without_builder, so a build form made the stored scene, and build_scene_on_device sets have_perm with built_by, the full upload clears both)
    if (permille == 0 || !have || !ctx->have_cost || !ctx->have_perm || !(cost > static_cast<double>(permille) / 1000.0 * base)) {
        fail(ctx, RVPT_HIP_OK, "%s: cost %.17g, base cost %.17g, limit %u permille: refitted", row.report, cost, base, permille);
        return RVPT_HIP_OK;
    }
    const size_t n_tris = ctx->n_tris;
    const uint32_t n = static_cast<uint32_t>(n_tris);
    const int built_by = ctx->built_by;
    const bool carry_rest = row.guard_carries_rest;
    if (int rc = grow(ctx, ctx->d_carry, ctx->cap_carry, n_tris * 4u, sizeof(float4))) return rc;
    if (carry_rest)
        if (int rc = grow(ctx, ctx->d_rest_carry, ctx->cap_rest_carry, n_tris * 3u, sizeof(float4))) return rc;
    const uint32_t rest_blocks = static_cast<uint32_t>((3ull * n + 255u) / 256u);
    hipLaunchKernelGGL(rv::carry_back_triangles, dim3(static_cast<uint32_t>((4ull * n + 255u) / 256u)), dim3(256), 0, ctx->stream, ctx->d_tris, ctx->d_perm, n, ctx->d_carry);
    if (carry_rest) hipLaunchKernelGGL(rv::rest_to_caller_order, dim3(rest_blocks), dim3(256), 0, ctx->stream, ctx->d_rest, ctx->d_perm, n, ctx->d_rest_carry);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (carry_rest) ctx->have_rest = false;  // (d_rest is in the order of a permutation that is about to go: an error below leaves no rest pose)
    if (int rc = build_scene_on_device(ctx, reinterpret_cast<const rvpt_triangle *>(ctx->d_carry), n_tris, ctx->host_mats.data(), ctx->host_mats.size(), built_by == rvpt_hip_ctx::kBuiltPloc,
                                       built_by == rvpt_hip_ctx::kBuiltSah))
        return rc;  // the build form's rule: its message, and no scene after anything but a bad material index (which stored rows cannot hold)
    // A PLOC build that fell back has left its sentence and built_by == kBuiltPloc: the scene then holds the LBVH tree, and the next rebuild is a PLOC build
    // again.  The pose and skin forms' report names the tree the scene holds (lbvh), the plain form's names the builder that ran (ploc): each as the header and
    // tests/_scene_model.py state it for that form, kept apart by the row's guard_names_tree.
    const bool fell_back = built_by == rvpt_hip_ctx::kBuiltPloc && !ctx->err.empty();
    if (carry_rest) {
        hipLaunchKernelGGL(rv::rest_to_stored_order, dim3(rest_blocks), dim3(256), 0, ctx->stream, ctx->d_rest_carry, ctx->d_perm, n, ctx->d_rest);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->have_rest = true;
    }
    static const char *const kNames[] = {"", "lbvh", "ploc", "sah"};
    fail(ctx, RVPT_HIP_OK, "%s: cost %.17g, base cost %.17g, limit %u permille: rebuilt (%s), new base cost %.17g", row.report, cost, base, permille,
         kNames[row.guard_names_tree && fell_back ? rvpt_hip_ctx::kBuiltLbvh : built_by], ctx->base_cost);
    return RVPT_HIP_OK;
}

// The order, for a form of two halves under its plain or its guarded count.  The form's own refusals come first, in its words and its order: `validate`
// touches nothing stored and says whether the context holds a tree.  Then the guard's refusal, before anything of the stored scene is touched; then the form:
// `execute` refuses nothing a caller's arguments decide; then the guard's tail.  Brute-force contexts hold no tree: there a guarded count is the plain form.
template <typename Validate, typename Execute>
static int run_guardable(rvpt_hip_ctx *ctx, const rv::SceneCall &call, Validate validate, Execute execute)
{
    const rv::SceneFormRow &row = rv::scene_form_row(call.form);
    bool bvh = false;
    if (int rc = validate(&bvh)) return rc;
    const bool guarded = row.report && bvh;
    if (guarded)
        if (int rc = refuse_limit_without_builder(ctx, call)) return rc;
    if (int rc = execute()) return rc;
    return guarded ? guarded_tail(ctx, row, call.permille) : RVPT_HIP_OK;
}

// The GUARDED UPDATE: the update form, which is one piece and makes its refusals itself, under the guard.  Its refusals of a missing scene and of another count
// come first and in its words, then the guard's.
static int update_geometry_guarded(rvpt_hip_ctx *ctx, const rv::SceneCall &call, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t n_mats)
{
    if (mats || n_mats) return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded update takes no materials: it keeps the stored ones");
    if (n_tris == 0) return fail(ctx, RVPT_HIP_ERR_INVALID, "guarded update without triangles");
    if (!is_bvh(ctx, n_tris)) {  // no tree to cost: the plain update form
        const int rc = update_geometry(ctx, tris, n_tris);
        if (rc == RVPT_HIP_OK) ctx->err.clear();
        return rc;
    }
    if (ctx->have_scene && n_tris == ctx->n_tris)
        if (int rc = refuse_limit_without_builder(ctx, call)) return rc;
    if (int rc = update_geometry(ctx, tris, n_tris)) return rc;
    return guarded_tail(ctx, rv::scene_form_row(call.form), call.permille);
}

// The FULL UPLOAD: the caller's tree (BVH contexts), triangles in its leaf order, materials.
static int upload_full(rvpt_hip_ctx *ctx, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris, size_t n_tris, const rvpt_material *mats, size_t n_mats)
{
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

}  // namespace

int rvpt_hip_upload_scene(rvpt_hip_ctx *ctx, const rvpt_bvh_node *nodes, size_t n_nodes, const rvpt_triangle *tris,
                          size_t n_tris, const rvpt_material *mats, size_t n_mats)
{
    using rv::SceneForm;
    if (!ctx) return fail(nullptr, RVPT_HIP_ERR_INVALID, "ctx is NULL");
    const rv::SceneCall call = rv::classify_scene_call(nodes != nullptr, n_nodes, tris != nullptr, n_tris, mats != nullptr, n_mats);
    const rv::SceneFormRow &row = rv::scene_form_row(call.form);
    // the forms that take the scene's arrays check them here; under the pose, bind and skin counts `nodes` is the form's own list and `tris` must be NULL: those
    // forms refuse their arguments themselves, in their own words and order (and behind the limit of a guarded count)
    switch (call.form) {
    case SceneForm::Pose: case SceneForm::PoseGuarded: case SceneForm::BindSkin: case SceneForm::Skin: case SceneForm::SkinGuarded:
        break;
    default:
        if ((n_tris && !tris) || (n_mats && !mats)) return fail(ctx, RVPT_HIP_ERR_INVALID, "NULL scene array");
        if (n_tris > 0x3FFFFFFFull) return fail(ctx, RVPT_HIP_ERR_INVALID, "too many triangles");
    }
    if (!call.limit_ok)
        return fail(ctx, RVPT_HIP_ERR_INVALID, "%s: the limit is 0 (report only) or 1000 .. 65535 permille, got %zu", row.report, static_cast<size_t>(call.permille));
    int rc = RVPT_HIP_OK;
    switch (call.form) {
    case SceneForm::Upload:
        rc = upload_full(ctx, nodes, n_nodes, tris, n_tris, mats, n_mats);
        break;
    case SceneForm::BuildLbvh: case SceneForm::BuildPloc: case SceneForm::BuildSah:
        // BVH contexts build the tree on the device; brute-force contexts (and an empty scene) ignore nodes and n_nodes as ever: the ordinary upload
        rc = is_bvh(ctx, n_tris) ? build_scene_on_device(ctx, tris, n_tris, mats, n_mats, call.form == SceneForm::BuildPloc, call.form == SceneForm::BuildSah)
                                 : upload_full(ctx, nullptr, 0, tris, n_tris, mats, n_mats);
        break;
    case SceneForm::Update:  // triangles without nodes and without materials (as a full upload it could never succeed: no material index fits n_mats == 0)
        rc = update_geometry(ctx, tris, n_tris);
        break;
    case SceneForm::UpdateGuarded:
        rc = update_geometry_guarded(ctx, call, tris, n_tris, mats, n_mats);
        break;
    case SceneForm::UpdateSparse:  // `nodes` points at n_tris indices (n_tris == 0 arrives here too: the form says so itself)
        rc = update_geometry_sparse(ctx, reinterpret_cast<const uint32_t *>(nodes), tris, n_tris, mats, n_mats);
        break;
    case SceneForm::Pose: case SceneForm::PoseGuarded: {  // `nodes` points at n_tris rvpt_part_move records
        const rvpt_part_move *const moves = reinterpret_cast<const rvpt_part_move *>(nodes);
        PoseList list;
        rc = run_guardable(
            ctx, call, [&](bool *bvh) { const int r = pose_validate(ctx, moves, tris, n_tris, mats, n_mats, &list); *bvh = list.bvh; return r; },
            [&] { return pose_execute(ctx, moves, n_tris, list); });
        break;
    }
    case SceneForm::BindSkin:  // `nodes` points at three rvpt_vertex_skin records per triangle
        rc = bind_skin(ctx, reinterpret_cast<const rvpt_vertex_skin *>(nodes), tris, n_tris, mats, n_mats);
        break;
    case SceneForm::Skin: case SceneForm::SkinGuarded: {  // `nodes` points at n_tris rvpt_bone matrices
        const rvpt_bone *const bones = reinterpret_cast<const rvpt_bone *>(nodes);
        SkinList list;
        rc = run_guardable(
            ctx, call, [&](bool *bvh) { const int r = skin_validate(ctx, bones, tris, n_tris, mats, n_mats, &list); *bvh = list.bvh; return r; },
            [&] { return skin_execute(ctx, bones, n_tris, list); });
        break;
    }
    }
    // What the call leaves of the binding and of the rest pose (include/rvpt_hip.h; tests/_scene_model.py): a successful call by its form's row — the update forms
    // keep the binding, a full upload and a build form the caller asks for drop it; the rest pose is the stored vertices as the last successful call of any form
    // but the pose and skin forms and the bind left them, so after any other the next pose update snapshots afresh — and a call that leaves no scene (a build or
    // a guard's rebuild that failed) drops both.
    if ((rc == RVPT_HIP_OK && !row.keeps_binding) || !ctx->have_scene) ctx->have_skin = false, ctx->skin_bones = 0;
    if ((rc == RVPT_HIP_OK && !row.keeps_rest) || !ctx->have_scene) ctx->have_rest = false;
    return rc;
}
