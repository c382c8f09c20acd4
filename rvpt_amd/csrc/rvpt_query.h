// rvpt_query.h — ray queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_RAY_HITS): closest and any hit for a caller's rays, in place.  The kernels live in
// rvpt_query.hip; rvpt_abi.hip validates, stages host records and owns the buffers.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rv {

// Which walk answers a context's queries (one order per kind of context, never the nearer-child-first order):
//   Wide   — intersect_bvh (intersection.glsl:361-413) over the 4-wide form of the tree, where the context holds one (rvpt_bvh4.hip's per-lane walk)
//   Binary — the same traversal over the binary nodes: heads that do not pack, a wide stack past 4096 slots, the laboratory's caller-layout knob
//   Brute  — triangles 0 .. n-1 in stored order (brute-force contexts, and the empty scene of any context)
enum class QueryKind : uint32_t { Wide = 0, Binary = 1, Brute = 2 };

constexpr uint32_t kQueryRecordBytes = 48;   // sizeof(rvpt_ray_hit): three float4
constexpr uint32_t kQueryLdsLevels = 8;      // stack slots per lane kept in LDS (16 KiB per work-group); deeper ones go to one global column per thread and level
constexpr uint32_t kQueryTopNodes = 64;      // wide nodes from the top of the (breadth-first) tree copied into LDS: 8 KiB
constexpr uint32_t kQueryTileTris = 512;     // prepared triangles per LDS tile of the brute-force kernel: 32 KiB
constexpr uint32_t kQueryMaxHits = 8;        // RVPT_HIP_RAY_MAX_HITS: the k of a k-nearest query, held in register lists of 2, 4 or 8 slots
constexpr size_t kQueryStackMaxBytes = size_t(256) << 20;  // the global part of the stack never takes more: the persistent grid shrinks instead

struct QueryScene {
    QueryKind kind;
    const float4 *prep;    // n_tris x 4 float4, prepared triangles
    const float4 *nodes;   // binary nodes, 2 float4 each (Wide: the root's box; Binary: the tree)
    const float4 *wide;    // Wide: 8 float4 per node
    const uint32_t *perm;  // non-null: prim = perm[stored index] (the caller's numbering after a build form)
    const float4 *unit_n;  // n_tris: (normalize(n), 0) by stored index — read by crossing queries alone
    uint32_t n_tris, n_wide, head_shift;
    uint32_t stack_levels;  // slots a walk can hold at once (Wide: wide_stack_levels; Binary: the tree's height)
};

struct QueryPlan {
    uint32_t grid;         // work-groups of kBlock threads
    uint32_t lds_levels;   // stack slots per lane in LDS
    uint32_t top_nodes;    // Wide: nodes copied into LDS
    size_t lds_bytes;      // dynamic LDS per work-group
    size_t stack_words;    // uint32 words of the global part of the stack (0: none); the launch also needs one claim word, which precedes them
};

// What a ray query gathers along its walk: Hits — the closest or any hit (RVPT_HIP_FORMAT_RAY_HITS), with k > 1 the k nearest hits
// (RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k)) —, or Crossings — one rvpt_ray_crossings per ray (RVPT_HIP_FORMAT_RAY_CROSSINGS; k is 1, scene.unit_n must be set).
enum class QueryForm : uint32_t { Hits = 0, Crossings = 1 };

// The launch shape for n records: a persistent grid sized from occupancy for the tree walks (the overflow stack is bounded by the grid, not by n), one
// work-group per 256 records for the brute-force kernel.  k > 1: n counts GROUPS of k records, one ray each.  The occupancy is that of the instance the
// launch will use.
hipError_t query_plan(const QueryScene &scene, QueryForm form, uint32_t n, int num_cus, QueryPlan *plan, uint32_t k = 1);
// Answers records[0 .. n) in place on `stream` — with k > 1 the n groups records[0 .. n * k), the plan made with the same form and k.  `scratch` holds 64 words
// (the first is the claim counter, zeroed here) followed by plan.stack_words words.
hipError_t query_launch(hipStream_t stream, const QueryScene &scene, QueryForm form, const QueryPlan &plan, uint32_t *scratch, void *records, uint32_t n, uint32_t k = 1);

}  // namespace rv
