// rvpt_build.h — the device BVH build (rvpt_build.hip), launched by rvpt_hip_upload_scene's BUILD FORM (rvpt_scene.hip: build_scene_on_device): triangles in the
// caller's order in, the binary tree in its breadth-first device layout, its level table and its 4-wide form out.  Nothing derived from the triangles visits
// the host except a few counters.
//
// THE TREE (one specification, written twice: here for the device, rvpt_amd/scene.py: build_lbvh in numpy — the two give the same topology, which is what
// tests/test_device_build.py compares bit for bit):
//   key of triangle i (caller's index):  c = (v0 + v1 + v2) * (1.0f / 3.0f) per axis, float32, left to right, no contraction (as bvh_builder.cpp);
//       lo, hi = min, max of the centroids per axis (exact; NaN centroids take no part);
//       q = clamp((int)((c - lo) * (1024.0f / (hi - lo))), 0, 1023) with the IEEE float32 divide — evaluated as f >= 1023 ? 1023 : f >= 0 ? (int)f : 0, so that
//       a NaN (every comparison fails) gives 0 and an infinity 1023 without leaning on an undefined conversion; q = 0 on an axis whose extent is not > 0;
//       code = 30-bit Morton code, x the highest bit of each triple; key = code << 32 | i.  Keys are unique: the ascending sort is unique.
//   nodes: a node is a range [a, b] of the sorted keys; a leaf iff b - a + 1 <= kLbvhLeafTris; otherwise p = the highest bit in which key[a] and key[b]
//       differ and the right child starts at the first s in (a, b] whose bit p is set (the keys are sorted: bit p is 0 .. 0 1 .. 1 over the range).
//   height: a split on a code bit can happen at most 30 times along a path, a split on an index bit at most ceil(log2 n) times (p strictly falls), then the
//       leaf: at most 30 + ceil(log2 n) + 1 <= 61 levels for n <= 2^30 triangles, so every such tree fits rv::kBvhStackDepth (64).  The build counts the
//       levels it makes and fails with a message rather than clamp.
//
// THE PLOC TREE (RVPT_HIP_NODES_BUILD_PLOC; rvpt_ploc.hip on the device, rvpt_amd/scene.py: build_ploc in numpy — the same topology, compared bit for bit by
// tests/test_device_build_ploc.py): parallel locally-ordered clustering (Meister & Bittner 2018), bottom-up merging over the order above.
//   order: keys, sort and perm are exactly the LBVH's; triangle j of the leaf order is sorted key j.
//   start: one cluster per sorted triangle, its box the exact min / max of its nine vertex coordinates (fminf / fmaxf: a NaN coordinate takes no part).
//   one iteration over the m clusters in array order: cluster i takes, among the j != i with |i - j| <= kPlocRadius, the minimum of the triple
//       (d(i, j), i xor j, min(i, j)).  d = the half-area of the union box in double: e = (double)hi - (double)lo per axis, (ex ey + ey ez) + ez ex, no
//       contraction; a d that is not finite counts as +inf.  The triple is symmetric in (i, j) and totally ordered, so the globally smallest pair is mutual
//       and every iteration merges at least one pair.  The xor term makes runs of equal distances pair up as buddies (0-1, 2-3, ..): by min(i, j) alone only
//       the first pair of such a run would be mutual, one merge per iteration, a chain.  Every mutual pair i < j becomes one inner node at position i (left
//       child cluster i, right child cluster j, box = min / max of the two); position j is removed; the array is compacted in order.  Until one cluster is left.
//   layout: the finished tree is laid out from the root, level by level: root at 0, slot 1 unused, the children of the k-th inner node of a level (in node
//       index order) at next_begin + 2 k and + 2 k + 1; a leaf is count = 1, first = its sorted position.  Boxes: refit_level, as after the LBVH.
//   bounds on trouble: PLOC promises neither a height nor an iteration count.  A tree of more than kPlocMaxHeight levels (62: the depth the BVH checks of the
//       tests allow, inside the 64 the traversal stack walks), or one that is not finished after kPlocMaxIterations iterations, is dropped and the call
//       builds the LBVH tree above from the same sorted keys.  A rule, not an error: rvpt_hip_last_error then says so (and is empty after a PLOC tree).
//
// THE SAH TREE (RVPT_HIP_NODES_BUILD_SAH; rvpt_sah.hip on the device, rvpt_amd/scene.py: build_sah in numpy — the same topology, compared bit for bit by
// tests/test_device_build_sah.py): a restatement of build_tree in bvh_builder.cpp, level by level, with every unstable step made stable, so that node for node
// the triangle sets and the boxes are rvpt_bvh_build's (tests/test_sah_host.py); only the order of triangles inside a leaf may differ (std::partition and
// std::nth_element are unstable).  kSahBins = 16, kSahMinLeaf = 2, kSahMaxLeaf = 8, kSahBalanceDepth = 30, traversal cost 0: the device ignores
// RVPT_BVH_TRAVERSAL_COST, which only the host builder reads.
//   per triangle i (caller's index): box = fminf / fmaxf of the three vertices; centroid = (v0 + v1 + v2) * (1.0f / 3.0f), float32, left to right, no
//       contraction; the index array starts as 0 .. n - 1.
//   per node (a range of the index array, depth = its level): bounds and cbounds (of the centroids) are exact min / max, a NaN takes no part (a side nothing
//       took part in stays +-FLT_MAX, the host's empty Box; and as that Box starts at +-FLT_MAX and takes std::min / std::max, a low side is never above
//       FLT_MAX and a high side never below -FLT_MAX: nothing but +inf on a low side gives FLT_MAX).  count < 2: a leaf.
//   binning (only where depth < 30): per axis 0, 1, 2 with extent = cbounds.hi - cbounds.lo > 0: scale = 16.0f / extent (the IEEE float32 divide);
//       bin = f >= 15 ? 15 : f >= 0 ? (int)f : 0 with f = (c - lo) * scale — the keys' rule above: a NaN gives 0, +inf gives 15, nothing leans on an undefined
//       conversion; bin boxes and counts are exact.  The right sweep and then the left sweep as in the host code: half_area = dx * (dy + dz) + dy * dz in
//       float32 on extents clamped at 0 (e < 0 ? 0 : e), cost = half_area * (float)count, FLT_MAX the sentinel of an empty right side; the winner is the FIRST
//       strict minimum in (axis, bin) order.
//   decision, with leaf_cost = half_area(bounds) * (float)count: a binned split if one was found and best_cost < leaf_cost; otherwise a leaf if count <= 8;
//       otherwise the median split; also the median split if the binned split leaves one side empty.
//   binned split: a STABLE partition, triangles with bin < best_bin go left and keep their relative order.
//   median split: the widest cbounds axis (the first strict maximum, starting from -1 as the host does); the whole range SORTED by (NaN last, centroid on
//       that axis with -0 == +0, caller's index); the left child takes the first count / 2.  (The host's nth_element selects the same sets.)
//   layout: breadth first as above: root at 0, slot 1 unused, the children of the k-th splitting node of a level at next_begin + 2 k and + 2 k + 1; a leaf is
//       (first = start of its range, count); perm = the final index array; boxes by refit_level.
//   height: a binned or median split leaves both sides non-empty, a median split halves: at most 30 + ceil(log2 n) + 1 levels.  The build counts its levels and
//       fails with a message rather than clamp.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rv {

// Triangles per leaf at most.  Started at 4; settled at 2 by the traversal measurement of DESIGN.md §5.6 (profiles/device_build.txt): one-frame launches at 1080p
// on leaves of <= 2 against <= 4 are a tie on the 1 M-triangle terrain (3 229 against 3 253 Msamples/s, inside the spread) and 11 % faster on Cornell + 9 k
// (1 821 against 1 642); leaves of <= 8 are 14 % and 30 % slower; the default scene cannot tell.  Morton order pairs neighbours, not good leaves: the fewer
// triangles a visited leaf drags in, the better.  (tools/build_bench.py traversal on a library built with -DRVPT_LBVH_LEAF_TRIS=4 / 8 is the comparison.)
#ifndef RVPT_LBVH_LEAF_TRIS
#define RVPT_LBVH_LEAF_TRIS 2
#endif
constexpr uint32_t kLbvhLeafTris = RVPT_LBVH_LEAF_TRIS;

// counters the build keeps on the device (one small buffer; read back a few words at a time)
enum BuildCounter : uint32_t {
    kBuildFirstBad = 0,
    kBuildMaxLeaf = 1,
    kBuildBounds = 2 /* .. 7: lo xyz, hi xyz as ordered integers */,
    kPlocRoot = 8 /* the provisional node of the PLOC tree's root */,
    kPlocIterations = 9 /* iterations in all; 0xFFFFFFFF: not finished within kPlocMaxIterations */,
    kSahSplits = 10 /* splitting nodes of the level just emitted */,
    kSahMedianTris = 11 /* triangles of median-split nodes, all levels so far */,
    kSahLargeNext = 12 /* large-node slots handed out, all levels so far */,
    kBuildCounters = 16
};

// The PLOC tree's constants (each stated a second time in rvpt_amd/scene.py).  Radius: 16 against 8 is profiles/EXPERIMENTS.md's entry.
#ifndef RVPT_PLOC_RADIUS
#define RVPT_PLOC_RADIUS 16
#endif
constexpr uint32_t kPlocRadius = RVPT_PLOC_RADIUS;
constexpr uint32_t kPlocMaxIterations = 256;
constexpr uint32_t kPlocMaxHeight = 62;
constexpr uint32_t kPlocTailClusters = 1024;  // not part of the tree: at most this many clusters are finished by one work-group in LDS (rvpt_ploc.hip: ploc_tail)

// Every function below enqueues on `stream` and returns the launch's error; none of them waits.
// src: reference Triangle records (four quads each) in the caller's order, DEVICE memory.

// the first triangle whose material index is outside [0, n_mats) -> counters[kBuildFirstBad] (0xFFFFFFFF: none); resets the counters
hipError_t build_validate_materials(hipStream_t stream, const float4 *src, uint32_t n_tris, uint32_t n_mats, uint32_t *counters);
// stage 1: centroid bounds (counters[kBuildBounds ..]) and the keys
hipError_t build_keys(hipStream_t stream, const float4 *src, uint32_t n_tris, uint32_t *counters, uint64_t *keys);
// stage 2: rocPRIM's radix sort of the keys (62 bits) and the exclusive scans of the level loops share one temporary buffer of this many bytes
hipError_t build_temp_bytes(uint32_t n_tris, size_t *bytes);
hipError_t build_sort_keys(hipStream_t stream, void *temp, size_t temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, uint32_t n_tris);
// stage 3: the 64-byte records gathered into leaf order, the permutation kept (perm[j] = caller's index of leaf-order triangle j)
hipError_t build_gather(hipStream_t stream, const float4 *src, const uint64_t *sorted_keys, uint32_t n_tris, float4 *tris_out, uint32_t *perm_out);
// the update form after a build form: vert0..vert2 (48 of every 64 bytes) of the caller's-order records gathered through the stored permutation
hipError_t build_gather_vertices(hipStream_t stream, const float4 *src, const uint32_t *perm, uint32_t n_tris, float4 *tris);
// stage 4, per level (root level first): ranges / flags describe the level's `count` nodes at device indices begin .. begin + count - 1 (flags[j] = the node
// splits; flags[count] = 0); the children go to next_begin + 2 * (number of splitting nodes before j) with their ranges / flags in ranges_next / flags_next.
// offs[count] = the number of splitting nodes when the stream gets there.  node_cap: quads-pairs d_nodes can hold (nothing is written beyond)
hipError_t build_root(hipStream_t stream, uint32_t n_tris, uint2 *ranges, uint32_t *flags, float4 *nodes);
hipError_t build_level(hipStream_t stream, void *temp, size_t temp_bytes, const uint64_t *sorted_keys, const uint2 *ranges, const uint32_t *flags, uint32_t *offs,
                       uint32_t begin, uint32_t count, uint32_t next_begin, uint2 *ranges_next, uint32_t *flags_next, float4 *nodes, uint32_t node_cap, uint32_t *counters);
// stage 7, the 4-wide form (bvh_wide.cpp: regroup, as a level loop): per wide level, `bin` = the binary inner nodes that become the wide nodes wbase .. wbase +
// count - 1.  Writes the d_wide_map rows, the leaf heads (heads: 4 words per wide node) and, behind the scan, the inner children's wide indices and bin_next.
// offs[count] = wide nodes of the next level.
hipError_t build_wide_root(hipStream_t stream, uint32_t *bin);
hipError_t build_wide_level(hipStream_t stream, void *temp, size_t temp_bytes, const float4 *nodes, uint32_t n_nodes, const uint32_t *bin, uint32_t wbase, uint32_t count,
                            uint32_t head_shift, uint32_t *cnt, uint32_t *offs, uint32_t *wide_map, uint32_t *heads, uint32_t wide_cap, uint32_t *bin_next);
// ... the head quads of the finished wide nodes (boxes: refit_wide_gather, on a zeroed buffer)
hipError_t build_wide_heads(hipStream_t stream, const uint32_t *heads, uint32_t n_wide, float *wide);
// ... and the stack need, per wide level, deepest first: need[w] = max over children i of (children - 1 - i) + need[inner child]
hipError_t build_wide_need(hipStream_t stream, const float *wide, uint32_t wbase, uint32_t count, uint32_t n_wide, uint32_t head_shift, uint32_t *need);


// The PLOC tree (rvpt_ploc.hip), between stage 3 and stage 5.  scratch: ploc_scratch_bytes(n) bytes, 8-byte aligned, kept until the layout is done.
size_t ploc_scratch_bytes(uint32_t n_tris);
// one cluster per leaf-order triangle (tris: the gathered records of stage 3) into half 0 of the double-buffered cluster array
hipError_t ploc_begin(hipStream_t stream, const float4 *tris, uint32_t n_tris, unsigned char *scratch);
// one iteration over the m clusters of half `parity`: nearest neighbours, keep flags, their scan (pos[m] = clusters left when the stream gets there), merge and
// compaction into the other half.  keep, pos: m + 1 words each
hipError_t ploc_iteration(hipStream_t stream, void *temp, size_t temp_bytes, unsigned char *scratch, uint32_t n_tris, uint32_t m, uint32_t parity, uint32_t *keep, uint32_t *pos);
// the last m <= kPlocTailClusters clusters of half `parity`, all remaining iterations in one work-group; `iterations` = those made so far.
// counters[kPlocRoot], counters[kPlocIterations] when the stream gets there
hipError_t ploc_finish(hipStream_t stream, unsigned char *scratch, uint32_t n_tris, uint32_t m, uint32_t parity, uint32_t iterations, uint32_t *counters);
// the layout, per level (root level first), the shape of build_root / build_level: cur = the provisional nodes of the level's `count` nodes, flags[j] = inner
hipError_t ploc_layout_root(hipStream_t stream, const uint32_t *counters, uint32_t n_tris, uint32_t *cur, uint32_t *flags, float4 *nodes);
hipError_t ploc_layout_level(hipStream_t stream, void *temp, size_t temp_bytes, const unsigned char *scratch, uint32_t n_tris, const uint32_t *cur, const uint32_t *flags, uint32_t *offs,
                             uint32_t begin, uint32_t count, uint32_t next_begin, uint32_t *cur_next, uint32_t *flags_next, float4 *nodes, uint32_t node_cap);


// The SAH tree's constants (each stated a second time in rvpt_amd/scene.py; the first four are bvh_builder.cpp's).
constexpr uint32_t kSahBins = 16, kSahMinLeaf = 2, kSahMaxLeaf = 8, kSahBalanceDepth = 30;
// not part of the tree: a node of more than kSahLargeNode triangles is reduced by several work-groups, each over kSahChunk positions of the index array, through
// global atomics; any other node by one wave in LDS.  kSahLargeNode >= kSahChunk is what lets a work-group meet at most two large nodes (rvpt_sah.hip: window_of).
constexpr uint32_t kSahLargeNode = 2048, kSahChunk = 2048;

// The SAH tree (rvpt_sah.hip), in place of stages 1 - 4.  scratch: sah_scratch_bytes(n) bytes, 16-byte aligned; temp: sah_temp_bytes (rocPRIM's scans and sorts).
size_t sah_scratch_bytes(uint32_t n_tris);
hipError_t sah_temp_bytes(uint32_t n_tris, size_t *bytes);
// boxes, centroids, the iota, the root level; resets counters[kBuildMaxLeaf] and the three kSah counters
hipError_t sah_begin(hipStream_t stream, const float4 *src, uint32_t n_tris, unsigned char *scratch, uint32_t *counters, float4 *nodes);
// (a), (b), (d) of one level: its `count` nodes at device indices begin .. begin + count - 1, read from half `parity` of the level arrays; `n_large` of them hold
// the large-node slots large_base .. large_base + n_large - 1.  counters[kSahSplits .. kSahLargeNext] when the stream gets there
hipError_t sah_decide_level(hipStream_t stream, void *temp, size_t temp_bytes, unsigned char *scratch, uint32_t n_tris, uint32_t parity, uint32_t depth, uint32_t begin, uint32_t count,
                            uint32_t next_begin, uint32_t large_base, uint32_t n_large, float4 *nodes, uint32_t node_cap, uint32_t *counters);
// (c) of that level: the index array of half `parity` partitioned into the other half; n_median: triangles of its median-split nodes
hipError_t sah_partition_level(hipStream_t stream, void *temp, size_t temp_bytes, unsigned char *scratch, uint32_t n_tris, uint32_t parity, uint32_t count, uint32_t n_median);
// stage 3 behind the tree: build_gather with the order taken from half `parity` of the index array
hipError_t sah_gather(hipStream_t stream, const float4 *src, const unsigned char *scratch, uint32_t n_tris, uint32_t parity, float4 *tris_out, uint32_t *perm_out);

}  // namespace rv
