// rvpt_nearest.h — point queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_NEAREST_POINTS): the nearest point of the mesh to a caller's points, in place.  The kernels
// live in rvpt_nearest.hip; rvpt_abi.hip validates, stages host records and owns the buffers (the ray queries' staging buffer and scratch: rvpt_query.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rvpt_query.h"

namespace rv {

constexpr uint32_t kNearestRecordBytes = 48;  // sizeof(rvpt_point_hit): three float4
constexpr uint32_t kNearestTileTris = 512;    // triangle rows (three vertex quads each) per LDS tile of the brute-force kernel: 24 KiB
constexpr uint32_t kNearestMaxK = 8;          // RVPT_HIP_POINT_MAX_NEAREST: the k of a k-nearest point query, held in register lists of 2, 4 or 8 slots

// The scene a point query asks: the vertex rows every update form keeps current, and on BVH contexts the binary nodes with their refitted boxes
struct NearestScene {
    bool brute;            // brute-force contexts, and the empty scene of any context
    const float4 *tris;    // n_tris x 4 float4: rvpt_triangle rows (d_tris), of which the walk reads vert0..2
    const float4 *nodes;   // n_nodes x 2 float4: the binary nodes
    const uint32_t *perm;  // non-null: prim = perm[stored index] (the caller's numbering after a build form)
    uint32_t n_tris, n_nodes;
    uint32_t stack_levels;  // slots a walk can hold at once: the tree's height
};

// The launch shape for n records (QueryPlan's fields as for ray queries; top_nodes is 0): a persistent grid sized from occupancy for the tree walk, one
// work-group per 256 records for the brute-force kernel.  k > 1 (RVPT_HIP_FORMAT_NEAREST_POINTS_K(k)): n counts GROUPS of k records, one point each, and the
// occupancy is that of the k-nearest instance the launch will use.
hipError_t nearest_plan(const NearestScene &scene, uint32_t n, int num_cus, QueryPlan *plan, uint32_t k = 1);
// Answers records[0 .. n) in place on `stream` — with k > 1 the n groups records[0 .. n * k), the plan made with the same k.  `scratch` as for query_launch:
// 64 words (the first is the claim counter, zeroed here), then plan.stack_words.
hipError_t nearest_launch(hipStream_t stream, const NearestScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, uint32_t n, uint32_t k = 1);

}  // namespace rv
