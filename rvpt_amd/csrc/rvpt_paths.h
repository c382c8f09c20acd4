// rvpt_paths.h — path queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_RAY_PATHS, RVPT_HIP_FORMAT_RAY_PATHS_MODE): an integrator's radiance along a caller's rays, in place.  The kernels live
// in rvpt_paths.hip; rvpt_abi.hip validates, stages host records and owns the buffers (the ray queries' staging buffer and scratch: rvpt_query.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rvpt_query.h"

namespace rv {

constexpr uint32_t kPathRecordBytes = 48;   // sizeof(rvpt_ray_path): three float4
constexpr uint32_t kPathMaxBounces = 1024;  // RVPT_HIP_PATH_MAX_BOUNCES: a record with a larger budget (or none) is invalid — no input makes a launch unbounded
constexpr uint32_t kPathModeKajiya = 9;     // RVPT_HIP_FORMAT_RAY_PATHS_MODE(9) = RVPT_HIP_FORMAT_RAY_PATHS: the lean kernels; modes 0 .. 8 run the GENERIC instances (shade_generic)
constexpr uint32_t kPathRun = 128;          // consecutive records a wave claims at once and deals to its lanes as their paths end
constexpr uint32_t kPathRefill = 32;        // tree walks: deal new segments once this many lanes of a wave wait for one (the frame kernels' bvh_refill)
constexpr uint32_t kPathLeafBatch = 16;     // 4-wide walk: run the parked leaves once this many lanes hold one (the frame kernels' bvh_leaf_batch)

// The scene a path is traced in: what a ray query walks (the kind chosen as for ray queries) and what shade() reads at a hit
struct PathScene {
    QueryScene walk;
    const uint32_t *mat_index;  // n_tris
    const float4 *unit_n;       // n_tris: (normalize(n), 0)
    const float4 *mats;         // n_mats x 3 float4, prepared (prepare_materials)
};

// The launch shape for n records: a persistent grid sized from occupancy for all three kinds (QueryPlan's fields as for ray queries; top_nodes and lds_levels
// are 0 for the brute-force kernel, whose LDS is one tile of kQueryTileTris prepared triangles).
// `mode` is the call's integrator, 0 .. kPathModeKajiya (a render mode of compute_pass.comp:76-95; Hart is not built): it picks the instance, whose own register
// count the grid is sized from, and path_launch must be given the same.
hipError_t path_plan(const PathScene &scene, uint32_t n, int num_cus, uint32_t mode, QueryPlan *plan);
// Answers records[0 .. n) in place on `stream`.  `scratch` as for query_launch: 64 words (the first is the claim counter, zeroed here), then plan.stack_words.
hipError_t path_launch(hipStream_t stream, const PathScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, uint32_t n, uint32_t mode);

}  // namespace rv
