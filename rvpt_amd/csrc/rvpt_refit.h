// rvpt_refit.h — the geometry update's kernels (rvpt_refit.hip), launched by rvpt_hip_upload_scene's update form (rvpt_scene.hip: update_geometry).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rv {

// the boxes of the binary nodes [begin, end) — one level of the breadth-first device layout — from their triangles (leaves) or their two children (inner
// nodes); launched level by level, deepest first.  tris: the reference Triangle records (four quads each), nodes: two quads each
__global__ void refit_level(float4 *__restrict__ nodes, uint32_t begin, uint32_t end, uint32_t n_nodes, const float4 *__restrict__ tris, uint32_t n_tris);
// ... then the wide nodes' copies of those boxes: map = 4 words per wide node (bvh_wide.h: build_wide_nodes' kid_map), n_slots = 4 x wide nodes
__global__ void refit_wide_gather(float *__restrict__ wide, const uint32_t *__restrict__ map, uint32_t n_slots, const float4 *__restrict__ nodes, uint32_t n_nodes);

// the tree cost of the guarded update (rvpt_refit.hip has the definition and what it relies on): stage one, one node per lane and one partial per work-group of
// kTreeCostBlock lanes (grid = ceil(n_nodes / kTreeCostBlock), partials holds that many doubles) ...
constexpr uint32_t kTreeCostBlock = 256;
__global__ void tree_cost_partials(const float4 *__restrict__ nodes, uint32_t n_nodes, double *__restrict__ partials);
// ... stage two, ONE work-group of kTreeCostBlock lanes: out[0] = cost, out[1] = the sum, out[2] = the root's half-area
__global__ void tree_cost_finish(const double *__restrict__ partials, uint32_t n_partials, const float4 *__restrict__ nodes, double *__restrict__ out);
// the triangles of d_tris carried back into the caller's order for a guarded rebuild: out[perm[pos]] = tris[pos], grid = ceil(4 n / block) (one thread per quad)
__global__ void carry_back_triangles(const float4 *__restrict__ tris, const uint32_t *__restrict__ perm, uint32_t n, float4 *__restrict__ out);

// The SPARSE UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h; rvpt_scene.hip: update_geometry_sparse).  refit_level for the flagged nodes of a level alone ...
__global__ void refit_level_dirty(float4 *__restrict__ nodes, uint32_t begin, uint32_t end, uint32_t n_nodes, const float4 *__restrict__ tris, uint32_t n_tris,
                                  uint32_t *__restrict__ dirty);
// ... the maps of a topology (both pre-filled with 0xFFFFFFFF; one thread per node) and the inverse of a build form's permutation (one thread per triangle) ...
__global__ void sparse_topology(const float4 *__restrict__ nodes, uint32_t n_nodes, uint32_t n_tris, uint32_t *__restrict__ parent, uint32_t *__restrict__ leaf_of);
__global__ void sparse_invert_permutation(const uint32_t *__restrict__ perm, uint32_t n, uint32_t *__restrict__ inv);
// ... the list's validation in two launches (one thread per entry; inv_perm may be null): the words it leaves, read back in one copy ...
enum : uint32_t { kSparseBadPosition = 0, kSparseDuplicate = 1, kSparseSpanLo = 2, kSparseSpanHi = 3, kSparseWords = 4 };
__global__ void sparse_claim(const uint32_t *__restrict__ indices, uint32_t k, uint32_t n_tris, const uint32_t *__restrict__ inv_perm, uint32_t *__restrict__ claim,
                             uint32_t *__restrict__ words);
__global__ void sparse_duplicates(const uint32_t *__restrict__ indices, uint32_t k, uint32_t n_tris, const uint32_t *__restrict__ claim, uint32_t *__restrict__ words);
// ... and the scatter of the vertex rows with the marking of their paths (one thread per entry of a validated list; src: four quads per entry, the fourth unread)
__global__ void sparse_scatter(const float4 *__restrict__ src, const uint32_t *__restrict__ indices, uint32_t k, uint32_t n_tris, const uint32_t *__restrict__ inv_perm,
                               float4 *__restrict__ tris, const uint32_t *__restrict__ leaf_of, const uint32_t *__restrict__ parent, uint32_t n_nodes,
                               uint32_t *__restrict__ dirty);

// The POSE UPDATE of rvpt_hip_upload_scene (include/rvpt_hip.h; rvpt_scene.hip: pose_validate, pose_execute): one thread per listed triangle of a validated list, blocks
// of 256.  rest: three quads per triangle in stored order; moves: k rvpt_part_move records as 16 words each; prefix: k + 1 exclusive sums of their counts,
// prefix[k] = total; inv_perm may be null.  Writes the vertex rows of tris and flags the paths as sparse_scatter does.
__global__ void pose_parts(const float4 *__restrict__ rest, const uint32_t *__restrict__ moves, const uint32_t *__restrict__ prefix, uint32_t k, uint32_t total,
                           uint32_t n_tris, const uint32_t *__restrict__ inv_perm, float4 *__restrict__ tris, const uint32_t *__restrict__ leaf_of,
                           const uint32_t *__restrict__ parent, uint32_t n_nodes, uint32_t *__restrict__ dirty);

// The GUARDED POSE UPDATE (include/rvpt_hip.h; rvpt_scene.hip: guarded_tail): the rest pose through a rebuild.  Three quads per triangle on both
// sides, one thread per quad, grid = ceil(3 n / block): out[perm[pos]] = rest[pos] with the old permutation in front of the build ...
__global__ void rest_to_caller_order(const float4 *__restrict__ rest, const uint32_t *__restrict__ perm, uint32_t n, float4 *__restrict__ out);
// ... and rest[pos] = in[perm[pos]] with the new one behind it
__global__ void rest_to_stored_order(const float4 *__restrict__ in, const uint32_t *__restrict__ perm, uint32_t n, float4 *__restrict__ rest);

// The SKIN UPDATE (include/rvpt_hip.h; rvpt_scene.hip: bind_skin, skin_validate, skin_execute).  skin_check: the check of a bind from device memory, one thread per
// 32-byte record, grid = ceil(n_records / block); words = {all ones, 0} before the launch, the smallest offence and the largest bone with its place after it ...
__global__ void skin_check(const uint4 *__restrict__ skin, uint64_t n_records, uint32_t limit, unsigned long long *__restrict__ words);
// ... and the skin: one thread per vertex quad of the rest pose at a time, ANY grid of kSkinBlock lanes (the work-groups stride over the 3 n quads; the host
// launches what the device holds at once), k x 48 bytes of dynamic LDS for the matrices (k <= 1024), staged once per work-group.  skin: two
// quads per vertex in the update form's order, bones: three quads per matrix, perm may be null.  Writes the three vertex rows of every triangle of tris.
constexpr uint32_t kSkinBlock = 256;
__global__ void skin_vertices(const float4 *__restrict__ rest, const uint4 *__restrict__ skin, const float4 *__restrict__ bones, uint32_t k, uint32_t n_tris,
                              const uint32_t *__restrict__ perm, float4 *__restrict__ tris);

}  // namespace rv
