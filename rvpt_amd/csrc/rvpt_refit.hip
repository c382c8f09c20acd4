// rvpt_refit.hip — the geometry update's kernels (rvpt_hip_upload_scene's update form: same topology, moved vertices): the boxes of the tree recomputed on the
// device.  Not frame kernels: this file is outside build.py's KERNEL_SOURCES, so the frame kernels' identity (kernel_sha) and the profiles stamped with it stand.
//
// min / max of floats is exact and order-independent, so the result is THE refit of the tree (rvpt_amd/scene.py: refit_bvh is the same in numpy), not an
// approximation of it.  (Only the sign of a zero bound may differ between two orders; a slab test cannot tell: (+-0 - o) * inv compares equal.)
// A NaN takes no part (fminf / fmaxf return the other operand; rvpt_build.h states the rule for the builders): a bound is NaN only where nothing but NaN
// took part — all of a leaf's coordinates on that axis, or both children's bounds — and refit_bvh says the same.  tests/test_device_state.py reads the
// boxes back and compares them byte for byte, non-finite vertices included.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvpt_refit.h"

namespace rv {

// One launch per level of the breadth-first device layout, deepest first, in stream order: a level is the index range [begin, end), children have higher
// indices than their parent and lie on deeper levels, so every box a thread reads was written by an earlier launch.  No atomics, no waiting on another
// work-group.  A node = two quads: (first, count, minx, maxx), (miny, maxy, minz, maxz); only the six bounds are written.
// (refit_node: the box of one node, shared by refit_level and the sparse update's refit_level_dirty.)
__device__ inline void refit_node(float4 *__restrict__ nodes, uint32_t i, uint32_t n_nodes, const float4 *__restrict__ tris, uint32_t n_tris)
{
    const float4 head = nodes[2 * i];
    const uint32_t first = __float_as_uint(head.x), count = __float_as_uint(head.y);
    float lo[3], hi[3];
    if (count > 0) {  // a leaf: its triangles' nine coordinates each
        if (first >= n_tris || count > n_tris - first) return;  // (upload_scene validated the ranges; a stray word must not become an address)
        const float4 a0 = tris[4 * first];
        lo[0] = hi[0] = a0.x, lo[1] = hi[1] = a0.y, lo[2] = hi[2] = a0.z;
        for (uint32_t t = first; t < first + count; ++t)
            for (uint32_t v = 0; v < 3; ++v) {
                const float4 p = tris[4 * t + v];
                lo[0] = fminf(lo[0], p.x), hi[0] = fmaxf(hi[0], p.x);
                lo[1] = fminf(lo[1], p.y), hi[1] = fmaxf(hi[1], p.y);
                lo[2] = fminf(lo[2], p.z), hi[2] = fmaxf(hi[2], p.z);
            }
    } else {  // an inner node: its two children, refitted by the launch before this one
        if (first <= i || first >= n_nodes - 1u) return;  // (children lie behind their parent in this layout)
        const float4 l0 = nodes[2 * first], l1 = nodes[2 * first + 1], r0 = nodes[2 * first + 2], r1 = nodes[2 * first + 3];
        lo[0] = fminf(l0.z, r0.z), hi[0] = fmaxf(l0.w, r0.w);
        lo[1] = fminf(l1.x, r1.x), hi[1] = fmaxf(l1.y, r1.y);
        lo[2] = fminf(l1.z, r1.z), hi[2] = fmaxf(l1.w, r1.w);
    }
    nodes[2 * i] = make_float4(head.x, head.y, lo[0], hi[0]);
    nodes[2 * i + 1] = make_float4(lo[1], hi[1], lo[2], hi[2]);
}

__global__ void refit_level(float4 *__restrict__ nodes, uint32_t begin, uint32_t end, uint32_t n_nodes, const float4 *__restrict__ tris, uint32_t n_tris)
{
    const uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end || i >= n_nodes) return;
    refit_node(nodes, i, n_nodes, tris, n_tris);
}

// The SPARSE UPDATE's form of the same launch (include/rvpt_hip.h): the same arithmetic for the nodes of the level that sparse_scatter flagged, and only for
// them; the flag is cleared for the next update.  Every other box of the level is left as it is.  The flags were written by an earlier launch on the stream.
__global__ void refit_level_dirty(float4 *__restrict__ nodes, uint32_t begin, uint32_t end, uint32_t n_nodes, const float4 *__restrict__ tris, uint32_t n_tris,
                                  uint32_t *__restrict__ dirty)
{
    const uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end || i >= n_nodes) return;
    if (dirty[i] == 0u) return;
    dirty[i] = 0u;
    refit_node(nodes, i, n_nodes, tris, n_tris);
}

// ... then the 4-wide form: slot s of wide node w holds a copy of the box of binary node map[4 w + s] (build_wide_nodes' grouping, kept from the full upload;
// 0xFFFFFFFF = unused slot).  One thread per slot; heads and padding are not touched.  Wide node = minx[4] maxx[4] miny[4] maxy[4] minz[4] maxz[4] head[4] pad[4].
__global__ void refit_wide_gather(float *__restrict__ wide, const uint32_t *__restrict__ map, uint32_t n_slots, const float4 *__restrict__ nodes, uint32_t n_nodes)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_slots) return;
    const uint32_t b = map[t];
    if (b >= n_nodes) return;
    const float4 q0 = nodes[2 * b], q1 = nodes[2 * b + 1];
    float *q = wide + static_cast<size_t>(t >> 2) * 32u + (t & 3u);
    q[0] = q0.z, q[4] = q0.w, q[8] = q1.x, q[12] = q1.y, q[16] = q1.z, q[20] = q1.w;
}

// ---- the tree cost (include/rvpt_hip.h: the guarded update) ------------------------------------------------------------------------------------------------------
// cost = (sum over the inner nodes of their half-area + sum over the leaves of half-area x triangle count) / the root's half-area: rvpt_amd/scene.py: tree_cost.
//
// RELIES ON the breadth-first device layout: the node array [0, n_nodes) holds the root at 0, the unused slot 1, and from 2 on the levels of the tree back to
// back, so EVERY slot but 1 is a node the root reaches and a flat pass over the array is a pass over the tree.  Established by rvpt_hip_upload_scene
// (rvpt_scene.hip), which copies a caller's tree into that layout node by reachable node — strays never arrive — and by build_scene_on_device, whose level
// loops hand out the slots pair by pair; both pass n_nodes = the end of the last level.  Slot 1 is skipped here by its index, whatever it holds.
//
// No atomics, and a fixed shape of additions: lane i of a wave holds node base + i, the wave folds its 64 terms with __shfl_down (32, 16, .. 1), lane 0 of
// wave 0 adds the work-group's four wave sums in wave order and writes ONE partial per work-group with a plain vector store; tree_cost_finish then adds the
// partials in index order.  The same tree gives the same 64 bits on every run.  Double precision: a node costs nine FP64 operations and
// the fold six more against 32 bytes read, so the pass is bound by reading the nodes once, not by the FP64 rate.

// the half-area of a box: its float32 bounds widened to double, the extents and everything after them in double, every operation rounded on its own (no
// contraction: the host statement has none)
__device__ inline double tree_cost_half_area(float4 q0, float4 q1)
{
    const double ex = __dsub_rn(static_cast<double>(q0.w), static_cast<double>(q0.z)), ey = __dsub_rn(static_cast<double>(q1.y), static_cast<double>(q1.x)),
                 ez = __dsub_rn(static_cast<double>(q1.w), static_cast<double>(q1.z));
    return __dadd_rn(__dadd_rn(__dmul_rn(ex, ey), __dmul_rn(ey, ez)), __dmul_rn(ez, ex));
}

__global__ __launch_bounds__(kTreeCostBlock) void tree_cost_partials(const float4 *__restrict__ nodes, uint32_t n_nodes, double *__restrict__ partials)
{
    __shared__ double wave_sum[kTreeCostBlock / 64];
    const uint32_t i = blockIdx.x * kTreeCostBlock + threadIdx.x;
    double term = 0.0;
    if (i < n_nodes && i != 1u) {
        const float4 q0 = nodes[2 * i], q1 = nodes[2 * i + 1];
        const uint32_t count = __float_as_uint(q0.y);
        term = tree_cost_half_area(q0, q1);
        if (count > 0) term = __dmul_rn(term, static_cast<double>(count));
    }
    for (int off = 32; off > 0; off >>= 1) term = __dadd_rn(term, __shfl_down(term, off, 64));
    if ((threadIdx.x & 63u) == 0) wave_sum[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (uint32_t w = 1; w < kTreeCostBlock / 64; ++w) s = __dadd_rn(s, wave_sum[w]);
        partials[blockIdx.x] = s;
    }
}

// ONE work-group: thread t adds the partials [t * chunk, (t + 1) * chunk) in index order, thread 0 then adds the kTreeCostBlock chunk sums in index order: index
// order throughout, with the one grouping fixed by n_partials.  out[0] = the cost (0 where the root's half-area is 0), out[1] = the sum, out[2] = the root's half-area.
__global__ __launch_bounds__(kTreeCostBlock) void tree_cost_finish(const double *__restrict__ partials, uint32_t n_partials, const float4 *__restrict__ nodes, double *__restrict__ out)
{
    __shared__ double chunk_sum[kTreeCostBlock];
    const uint32_t chunk = (n_partials + kTreeCostBlock - 1u) / kTreeCostBlock;
    const uint32_t begin = min(threadIdx.x * chunk, n_partials), end = min(begin + chunk, n_partials);
    double s = 0.0;
    for (uint32_t k = begin; k < end; ++k) s = __dadd_rn(s, partials[k]);
    chunk_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = chunk_sum[0];
        for (uint32_t t = 1; t < kTreeCostBlock; ++t) total = __dadd_rn(total, chunk_sum[t]);
        const double root = tree_cost_half_area(nodes[0], nodes[1]);
        out[0] = root > 0.0 ? total / root : 0.0;
        out[1] = total;
        out[2] = root;
    }
}

// The carry-back for a guarded rebuild: the 64-byte records of d_tris (leaf order: moved vertices, stored mat_id rows) into the caller's order,
// out[perm[pos]] = tris[pos].  perm is a bijection of [0, n) (the build's gather wrote it), so every row of `out` is written exactly once; a word that is
// not an index is dropped, never an address.  One thread per quad.
__global__ void carry_back_triangles(const float4 *__restrict__ tris, const uint32_t *__restrict__ perm, uint32_t n, float4 *__restrict__ out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t pos = t >> 2, q = t & 3u;
    if (pos >= n) return;
    const uint32_t dst = perm[pos];
    if (dst >= n) return;
    out[4 * static_cast<size_t>(dst) + q] = tris[4 * static_cast<size_t>(pos) + q];
}

// ---- the sparse update (include/rvpt_hip.h: SPARSE UPDATE) -----------------------------------------------------------------------------------------------------
// The maps a sparse update walks, made from the breadth-first node array once per topology: parent[node] (0xFFFFFFFF for the root and for slots no node
// owns) and leaf_of[triangle position] (0xFFFFFFFF where no leaf holds it; both arrays are filled with that word before the launch).  One thread per node;
// the same guards as refit_node: a stray word never becomes an address.
__global__ void sparse_topology(const float4 *__restrict__ nodes, uint32_t n_nodes, uint32_t n_tris, uint32_t *__restrict__ parent, uint32_t *__restrict__ leaf_of)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes || i == 1u) return;
    const float4 head = nodes[2 * i];
    const uint32_t first = __float_as_uint(head.x), count = __float_as_uint(head.y);
    if (count > 0) {
        if (first >= n_tris || count > n_tris - first) return;
        for (uint32_t t = first; t < first + count; ++t) leaf_of[t] = i;
    } else {
        if (first <= i || first >= n_nodes - 1u) return;
        parent[first] = i, parent[first + 1u] = i;
    }
}

// inv[perm[pos]] = pos: the caller's index of a build form -> the position in leaf order.  perm is a bijection of [0, n); a word that is not an index is dropped.
__global__ void sparse_invert_permutation(const uint32_t *__restrict__ perm, uint32_t n, uint32_t *__restrict__ inv)
{
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    const uint32_t j = perm[pos];
    if (j < n) inv[j] = pos;
}

// Validation, pass one (one thread per list entry; claim[] = n_tris words of 0xFFFFFFFF, words = kSparseWords words: 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0):
// an index outside [0, n_tris) lowers words[kSparseBadPosition] to its list position; every other entry claims its triangle with its list position (the
// smallest position wins) and widens the span [words[kSparseSpanLo], words[kSparseSpanHi]] of the positions in leaf order the list touches.
__global__ void sparse_claim(const uint32_t *__restrict__ indices, uint32_t k, uint32_t n_tris, const uint32_t *__restrict__ inv_perm, uint32_t *__restrict__ claim,
                             uint32_t *__restrict__ words)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0xFFFFFFFFu, lo = 0xFFFFFFFFu, hi = 0u;  // (no early return: every lane of the wave takes part in the fold below)
    if (j < k) {
        const uint32_t idx = indices[j];
        if (idx >= n_tris) {
            bad = j;
        } else {
            atomicMin(&claim[idx], j);
            const uint32_t pos = inv_perm ? inv_perm[idx] : idx;
            if (pos < n_tris) lo = hi = pos;
        }
    }
    // one atomic per wave and word instead of one per entry: thousands of entries would otherwise queue on three addresses
    for (int off = 32; off > 0; off >>= 1) {
        bad = min(bad, static_cast<uint32_t>(__shfl_down(bad, off, 64)));
        lo = min(lo, static_cast<uint32_t>(__shfl_down(lo, off, 64)));
        hi = max(hi, static_cast<uint32_t>(__shfl_down(hi, off, 64)));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (bad != 0xFFFFFFFFu) atomicMin(&words[kSparseBadPosition], bad);
        if (lo <= hi) {
            atomicMin(&words[kSparseSpanLo], lo);
            atomicMax(&words[kSparseSpanHi], hi);
        }
    }
}

// ... pass two, a launch of its own behind the first: an entry that lost its claim names an index that occurs twice; the smallest such index value.
__global__ void sparse_duplicates(const uint32_t *__restrict__ indices, uint32_t k, uint32_t n_tris, const uint32_t *__restrict__ claim, uint32_t *__restrict__ words)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const uint32_t idx = indices[j];
    if (idx < n_tris && claim[idx] != j) atomicMin(&words[kSparseDuplicate], idx);
}

// The scatter (one thread per entry of a VALIDATED list: in range, no index twice, so no two threads write one row): the 48 vertex bytes of src[j] into row
// pos of tris — the mat_id quad of the row stays — and the path from the leaf that holds pos to the root flagged.  atomicExch hands the old flag back: a
// thread that finds a node flagged stops, the thread that flagged it goes on to the root.  The flags are only read by later launches on the stream.
__global__ void sparse_scatter(const float4 *__restrict__ src, const uint32_t *__restrict__ indices, uint32_t k, uint32_t n_tris, const uint32_t *__restrict__ inv_perm,
                               float4 *__restrict__ tris, const uint32_t *__restrict__ leaf_of, const uint32_t *__restrict__ parent, uint32_t n_nodes,
                               uint32_t *__restrict__ dirty)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const uint32_t idx = indices[j];
    if (idx >= n_tris) return;
    const uint32_t pos = inv_perm ? inv_perm[idx] : idx;
    if (pos >= n_tris) return;
    const float4 a = src[4 * static_cast<size_t>(j)], b = src[4 * static_cast<size_t>(j) + 1], c = src[4 * static_cast<size_t>(j) + 2];
    float4 *row = tris + 4 * static_cast<size_t>(pos);
    row[0] = a, row[1] = b, row[2] = c;
    // (a path holds at most one node per level; the bound keeps a malformed map from looping)
    for (uint32_t node = leaf_of[pos], hops = 0; node < n_nodes && hops < 128u; node = parent[node], ++hops)
        if (atomicExch(&dirty[node], 1u) != 0u) break;
}

// ---- the pose update (include/rvpt_hip.h: POSE UPDATE) ---------------------------------------------------------------------------------------------------------
// One thread per listed triangle of a VALIDATED list (ranges in range, no two sharing a triangle, so no two threads write one row).  moves: k records of 16
// words (twelve floats of the matrix, first, count, two zero words); prefix: k + 1 words, the exclusive sums of the counts, prefix[k] = total.  Thread t finds
// its part p — the last one with prefix[p] <= t — by binary search and takes triangle first[p] + (t - prefix[p]): consecutive lanes, consecutive triangles, and
// the twelve floats are the same address across a wave wherever the wave lies inside one part.  The vertex rows are posed FROM THE REST POSE (three quads per
// triangle, stored order), never from tris; every product and every sum is rounded on its own (__fmul_rn / __fadd_rn: no contraction whatever the flags).
// The w lanes (the host-side face normal the live code never reads) are carried over from the rest pose; the mat_id quad of the row stays.
// The flagging is sparse_scatter's walk, made once per run of equal leaves inside a wave: a lane whose predecessor in the wave holds the same leaf leaves the
// walk to it.  The first lane of a wave, a lane behind one of another part, behind one past the end of the grid or behind one that was dropped always walks:
// their leaves differ or are 0xFFFFFFFF.  No early return before the shuffle: every lane of the wave takes part in it.
__device__ inline float4 pose_vertex(const float *__restrict__ m, float4 p)
{
    float4 q;
    q.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[0], p.x), __fmul_rn(m[1], p.y)), __fmul_rn(m[2], p.z)), m[3]);
    q.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[4], p.x), __fmul_rn(m[5], p.y)), __fmul_rn(m[6], p.z)), m[7]);
    q.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m[8], p.x), __fmul_rn(m[9], p.y)), __fmul_rn(m[10], p.z)), m[11]);
    q.w = p.w;
    return q;
}

__global__ __launch_bounds__(256) void pose_parts(const float4 *__restrict__ rest, const uint32_t *__restrict__ moves, const uint32_t *__restrict__ prefix, uint32_t k, uint32_t total,
                                                  uint32_t n_tris, const uint32_t *__restrict__ inv_perm, float4 *__restrict__ tris, const uint32_t *__restrict__ leaf_of,
                                                  const uint32_t *__restrict__ parent, uint32_t n_nodes, uint32_t *__restrict__ dirty)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t leaf = 0xFFFFFFFFu;
    if (t < total && k > 0u) {
        uint32_t lo = 0u, hi = k;  // prefix[lo] <= t < prefix[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (prefix[mid] <= t) lo = mid;
            else hi = mid;
        }
        const uint32_t *__restrict__ rec = moves + 16u * static_cast<size_t>(lo);
        const uint32_t j = t - prefix[lo];
        const uint32_t first = rec[12], count = rec[13];
        if (j < count && first < n_tris && j < n_tris - first) {  // (the host validated the ranges; a stray word must not become an address)
            const uint32_t idx = first + j;
            const uint32_t pos = inv_perm ? inv_perm[idx] : idx;
            if (pos < n_tris) {
                const float *__restrict__ m = reinterpret_cast<const float *>(rec);
                const float4 *__restrict__ src = rest + 3u * static_cast<size_t>(pos);
                const float4 a = src[0], b = src[1], c = src[2];
                float4 *row = tris + 4u * static_cast<size_t>(pos);
                row[0] = pose_vertex(m, a), row[1] = pose_vertex(m, b), row[2] = pose_vertex(m, c);
                leaf = leaf_of[pos];
            }
        }
    }
    const uint32_t before = static_cast<uint32_t>(__shfl_up(static_cast<int>(leaf), 1, 64));
    if (leaf >= n_nodes) return;
    if ((threadIdx.x & 63u) != 0u && before == leaf) return;
    // (a path holds at most one node per level; the bound keeps a malformed map from looping)
    for (uint32_t node = leaf, hops = 0; node < n_nodes && hops < 128u; node = parent[node], ++hops)
        if (atomicExch(&dirty[node], 1u) != 0u) break;
}

// ---- the guarded pose update (include/rvpt_hip.h: GUARDED POSE UPDATE) -----------------------------------------------------------------------------------------
// The rest pose goes with a rebuild: its 48 bytes per triangle (three quads, stored order of the OLD permutation) are scattered into the caller's order in front
// of the build, out[perm_old[pos]] = rest[pos], and gathered by the permutation the build wrote behind it, rest[pos] = in[perm_new[pos]].  Two buffers: neither
// step can be done in place.  One thread per quad, 16-byte loads and stores; thread t holds quad t of the side in STORED order, so that side — the read of the
// scatter, the write of the gather — runs along consecutive lanes, and the other side moves in runs of 48 bytes.  perm is a bijection of [0, n) (the build's
// gather wrote it), so the scatter writes every row exactly once; a word that is not an index is dropped, never an address.  No atomics, no LDS.
__global__ void rest_to_caller_order(const float4 *__restrict__ rest, const uint32_t *__restrict__ perm, uint32_t n, float4 *__restrict__ out)
{
    const size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t pos = t / 3u;
    if (pos >= n) return;
    const uint32_t q = static_cast<uint32_t>(t - 3u * pos);
    const uint32_t dst = perm[pos];
    if (dst >= n) return;
    out[3u * static_cast<size_t>(dst) + q] = rest[t];
}

__global__ void rest_to_stored_order(const float4 *__restrict__ in, const uint32_t *__restrict__ perm, uint32_t n, float4 *__restrict__ rest)
{
    const size_t t = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const size_t pos = t / 3u;
    if (pos >= n) return;
    const uint32_t q = static_cast<uint32_t>(t - 3u * pos);
    const uint32_t src = perm[pos];
    if (src >= n) return;
    rest[t] = in[3u * static_cast<size_t>(src) + q];
}

// ---- the skin update (include/rvpt_hip.h: BIND, SKIN UPDATE) ---------------------------------------------------------------------------------------------------
// The check of a bind from DEVICE memory, one thread per rvpt_vertex_skin record (eight words: bone[4], weight[4]; 3 n of them).  words[0] is lowered to the
// smallest key 4 position + j of a bone[j] >= limit — the smallest offending record position, then the smallest j in it; the host fetches the value itself only
// when it has to word the refusal —, words[1] is raised to the largest key bone << 32 | ~position of the bones below the limit: the largest bone index and the
// smallest record position that holds it.  The host fills words with {all ones, 0} and reads both back in one copy.  One atomic per wave and word, as in sparse_claim; no early return in front of the fold.
__global__ void skin_check(const uint4 *__restrict__ skin, uint64_t n_records, uint32_t limit, unsigned long long *__restrict__ words)
{
    const uint64_t r = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long bad = ~0ull, top = 0ull;
    if (r < n_records) {
        const uint4 b = skin[2 * r];
        const uint32_t bone[4] = {b.x, b.y, b.z, b.w};
        for (uint32_t j = 4; j-- > 0;) {
            if (bone[j] >= limit) bad = 4ull * r + j;
            else top = max(top, (static_cast<unsigned long long>(bone[j]) << 32) | (0xFFFFFFFFull - r));
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        bad = min(bad, static_cast<unsigned long long>(__shfl_down(bad, off, 64)));
        top = max(top, static_cast<unsigned long long>(__shfl_down(top, off, 64)));
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (bad != ~0ull) atomicMin(&words[0], bad);
        atomicMax(&words[1], top);
    }
}

// The skin itself: one thread per VERTEX QUAD of the rest pose at a time, t = 3 pos + v as in rest_to_*_order, so rest[t] is a 16-byte load consecutive across
// lanes.  The grid is one the device holds at once (the host sizes it: as many work-groups per CU as their LDS allows, eight at the most) and strides over
// the quads, so that the matrices are staged once per RESIDENT work-group and not once per 256 quads: with 1024 matrices a work-group per 256 quads staged
// 48 KiB to skin 12 KiB of vertices and measured 0.264 ms against 0.216 ms on 1 M triangles (profiles/skin_update.txt).
// The record of the vertex is skin[3 idx + v], idx = perm ? perm[pos] : pos (the binding is kept in the order the plain update form takes; perm[pos] is the
// caller's index of stored position pos), read as two 16-byte loads.  The k matrices are staged once per work-group into dynamic LDS, ROW MAJOR as they
// arrive (k x 12 floats): a matrix is three ds_read_b128, whose bank is (address / 4) mod 64, so the sixteen lanes of one LDS cycle conflict only where two
// DIFFERENT bones lie a multiple of 16 bones apart (12 b mod 64 runs through all sixteen 4-bank slots over sixteen consecutive bones), and lanes of one
// triangle or of neighbours share their bones and are served by broadcast.  A transposed layout would turn the three loads into twelve.
// The arithmetic is the header's: q_j = pose_vertex(M[bone[j]], p), out = ((w0 q0 + w1 q1) + w2 q2) + w3 q3 per component, every product and sum rounded on its
// own; all four influences are evaluated whatever their weight.  A bone index >= k, or a perm word >= n, drops the vertex: it never becomes an address (the
// bind refused such records; a stray word must not fault).  No atomics, no return in front of the barrier or inside the loop.  The w lane comes from the rest pose.
__global__ __launch_bounds__(kSkinBlock) void skin_vertices(const float4 *__restrict__ rest, const uint4 *__restrict__ skin, const float4 *__restrict__ bones, uint32_t k,
                                                            uint32_t n_tris, const uint32_t *__restrict__ perm, float4 *__restrict__ tris)
{
    extern __shared__ float4 staged[];  // 3 k quads
    for (uint32_t i = threadIdx.x; i < 3u * k; i += kSkinBlock) staged[i] = bones[i];
    __syncthreads();
    const float *__restrict__ m = reinterpret_cast<const float *>(staged);
    const uint64_t total = 3ull * n_tris, step = static_cast<uint64_t>(gridDim.x) * kSkinBlock;
    for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kSkinBlock + threadIdx.x; t < total; t += step) {
        const uint64_t pos = t / 3u;
        const uint32_t v = static_cast<uint32_t>(t - 3u * pos);
        const uint32_t idx = perm ? perm[pos] : static_cast<uint32_t>(pos);
        if (idx >= n_tris) continue;
        const float4 p = rest[t];
        const uint4 *__restrict__ rec = skin + 2u * (3u * static_cast<uint64_t>(idx) + v);
        const uint4 b = rec[0], wq = rec[1];
        if (b.x >= k || b.y >= k || b.z >= k || b.w >= k) continue;
        const float w0 = __uint_as_float(wq.x), w1 = __uint_as_float(wq.y), w2 = __uint_as_float(wq.z), w3 = __uint_as_float(wq.w);
        const float4 q0 = pose_vertex(m + 12u * b.x, p), q1 = pose_vertex(m + 12u * b.y, p), q2 = pose_vertex(m + 12u * b.z, p), q3 = pose_vertex(m + 12u * b.w, p);
        float4 out;
        out.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w0, q0.x), __fmul_rn(w1, q1.x)), __fmul_rn(w2, q2.x)), __fmul_rn(w3, q3.x));
        out.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w0, q0.y), __fmul_rn(w1, q1.y)), __fmul_rn(w2, q2.y)), __fmul_rn(w3, q3.y));
        out.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w0, q0.z), __fmul_rn(w1, q1.z)), __fmul_rn(w2, q2.z)), __fmul_rn(w3, q3.z));
        out.w = p.w;
        tris[4u * pos + v] = out;
    }
}

}  // namespace rv
