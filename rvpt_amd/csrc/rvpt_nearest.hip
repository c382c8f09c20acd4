// rvpt_nearest.hip — point queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_NEAREST_POINTS): a record comes in as a point and a squared bound and goes out as the
// nearest point of the mesh, its squared distance, the triangle, the barycentric pair and the Voronoi region that decided.
//
// THE ANSWER IS DEFINED WITHOUT A WALK (NEAREST POINTS at rvpt_hip_read; rvpt_amd/scene.py: closest_point_triangles / closest_points state it in numpy): every
// stored triangle i gets a candidate (d2_i, prim_i) from closest_point() below, and the answer is the lexicographically smallest candidate below
// (max_d2, 0xFFFFFFFF).  The arithmetic is binary32 with every product, sum and quotient rounded on its own: this translation unit is compiled with
// -ffp-contract=off and without fast-math like every other, there is no fma_() in this file, and the divisions are plain `/`, which hipcc expands to the
// correctly rounded IEEE quotient (v_div_scale / v_rcp / v_fma / v_div_fmas / v_div_fixup) — numpy's float32 divide is the yardstick, NOT div_dots (rvpt_math.h),
// whose refined reciprocal leaves the IEEE result outside the normal range.
//
// WHY ANY WALK GIVES THAT ANSWER.  closest_point() clamps its point q into the triangle's own box, so q lies in the box of every node above the triangle; with
// g = max(max(lo - p, p - hi), 0) per axis of a node's box, rounding is monotone, hence |p - q| >= g per axis IN FLOATS and box_d2 <= d2_i for every triangle
// under the node.  A walk that skips a node iff box_d2 > best (strict) never skips a candidate that could win or tie: the visiting order is free.
//
// One point per lane.  nearest_bvh2 walks the BINARY nodes — the form every update keeps current — on the ray queries' persistent grid: waves claim runs of 64
// records, the first stack levels per lane live in LDS and the rest in one global column per thread of the grid (rvpt_query.hip).  The nearer child by box_d2
// goes first, the farther is stacked with its box_d2 and popped only while box_d2 <= best still holds.  nearest_brute streams the vertex rows through LDS in tiles.
// A record is three float4; the second and third (the out fields) are stored.  An index read from the tree never becomes an address unchecked.
//
// K-NEAREST POINTS (RVPT_HIP_FORMAT_NEAREST_POINTS_K(k), k > 1; scene.py: closest_points_k): the first k candidates of the same total order.  nearest_bvh2_k<CAP>
// and nearest_brute_k<CAP> are the two kernels above with `best` replaced by a sorted list of CAP (d2, stored index) pairs a lane keeps in VGPRs, and by `bound`:
// max_d2 until slot k - 1 is taken, then that entry's d2.  The prune stays NON-strict, a node is skipped iff box_d2 > bound, and a candidate is offered iff
// d2 <= bound, so a tie at the k-th distance with a smaller number still gets in.  THE PROOF IS THE SAME ONE: every triangle under a skipped node has
// d2_i >= box_d2 > bound, and bound only ever shrinks, so such a triangle could neither enter the list nor tie into it.  Each stored triangle is
// taken to lie under one leaf; a caller's tree that lists it under two may report it twice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rvpt_device.h"
#include "rvpt_nearest.h"
#include "rvpt_walk.h"

namespace rv {

namespace {

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;

struct NearestArgs {
    const float4 *tris, *nodes;
    const uint32_t *perm;
    float4 *records;
    uint32_t n, n_runs;          // records, runs of 64 records
    uint32_t *counter;           // the next run to claim (0 at launch)
    uint32_t *stack_overflow;    // [stack_levels - lds_levels][2][threads of the grid]
    uint32_t n_tris, n_nodes, stack_levels, lds_levels;
};

struct NearestPoint {
    f3 p;
    uint32_t max_bits;
    bool valid;
};

__device__ __forceinline__ bool finite_(const float x) { return __builtin_fabsf(x) < kInf; }  // false for NaN and +-inf

// (closest_point() itself is rvpt_nearest.h's: the sphere sweeps of rvpt_sweep.h call it too)
__device__ __forceinline__ Closest closest_point_row(const float4 *row, const f3 p)
{
    const float4 a = row[0], b = row[1], c = row[2];
    return closest_point(mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), p);
}

// box_d2 of a binary node's box (bounds = {minx,maxx,miny,maxy,minz,maxz}: n0.zw = x, n1.xy = y, n1.zw = z) in the expression shape of d2
__device__ __forceinline__ float box_d2(const f3 p, const float4 n0, const float4 n1)
{
    const float gx = __builtin_fmaxf(__builtin_fmaxf(n0.z - p.x, p.x - n0.w), 0.0f);
    const float gy = __builtin_fmaxf(__builtin_fmaxf(n1.x - p.y, p.y - n1.y), 0.0f);
    const float gz = __builtin_fmaxf(__builtin_fmaxf(n1.z - p.z, p.z - n1.w), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

__device__ __forceinline__ uint32_t reported(const uint32_t *perm, const uint32_t i) { return i == kNoPrim ? kNoPrim : (perm ? perm[i] : i); }

// (d2, prim of stored triangle i) against (best, prim of best_i), lexicographically; a NaN d2 passes neither comparison.  The perm words are loaded only on a tie.
__device__ __forceinline__ void accept(const uint32_t *perm, const float d2, const uint32_t i, float &best, uint32_t &best_i)
{
    if (d2 < best) {
        best = d2;
        best_i = i;
    } else if (d2 == best) {
        if (reported(perm, i) < reported(perm, best_i)) best_i = i;
    }
}

// A record's in fields.  A point with a non-finite component is a miss before any walk; so is a max_d2 that is NaN or below zero (-0.0 is zero).
__device__ __forceinline__ NearestPoint load_point(const float4 *records, const size_t r, const bool live)
{
    NearestPoint q;
    const float4 a = live ? records[3 * r + 0] : make_float4(0.f, 0.f, 0.f, 0.f);
    q.p = mk(a.x, a.y, a.z);
    q.max_bits = __float_as_uint(a.w);
    q.valid = live && finite_(a.x) && finite_(a.y) && finite_(a.z) && a.w >= 0.0f;
    return q;
}

// A record's out fields.  The winner's candidate is recomputed from its row (the same operations on the same operands: d2 has the bits the walk compared),
// which is cheaper than carrying eight more registers through the walk.
__device__ __forceinline__ void store_point(float4 *records, const size_t r, const NearestPoint &q, const float4 *tris, const uint32_t *perm, const uint32_t best_i)
{
    float4 out1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(q.max_bits));
    float4 out2 = make_float4(__uint_as_float(kNoPrim), 0.0f, 0.0f, __uint_as_float(0u));
    if (best_i != kNoPrim) {
        const Closest c = closest_point_row(tris + 4 * static_cast<size_t>(best_i), q.p);
        out1 = make_float4(c.q.x, c.q.y, c.q.z, c.d2);
        out2 = make_float4(__uint_as_float(reported(perm, best_i)), c.u, c.v, __uint_as_float(c.region));
    }
    records[3 * r + 1] = out1;
    records[3 * r + 2] = out2;
}

// K-NEAREST POINTS.  n, n_runs of NearestArgs count GROUPS of k records: record 0 of a group carries the point, record j receives the j-th entry.
struct NearestKArgs {
    NearestArgs q;
    uint32_t k;  // entries per point, 2 .. CAP (wave-uniform)
};

// CAP slots of (d2, stored index), sorted lexicographically by (d2, reported prim); an empty slot is (+inf, kNoPrim), which no candidate is above, so empty
// slots come last.  Slots at and past k fill like the others (entries pushed down past the k-th); nothing reads them.  Constant indices only, every loop
// unrolled: the list stays in VGPRs.
template <int CAP>
struct NearList {
    float d2[CAP];
    uint32_t index[CAP];
    float bound;  // max_d2, or the k-th d2 once slot k - 1 is taken

    __device__ __forceinline__ void reset(const float max_d2)
    {
#pragma unroll
        for (int j = 0; j < CAP; ++j) d2[j] = kInf, index[j] = kNoPrim;
        bound = max_d2;
    }
    // In front of the first entry the candidate (d, prim of i) is lexicographically smaller than, the rest one slot down, the last dropped.  The perm words are
    // loaded only by a lane with a d2 tie (accept() above).  From the last slot up, so that slot j - 1 is still the old one when slot j takes it.
    __device__ __forceinline__ void insert(const uint32_t *perm, const bool offer, const float d, const uint32_t i, const float max_d2, const uint32_t k)
    {
        bool tie = false;
#pragma unroll
        for (int j = 0; j < CAP; ++j) tie = tie || d == d2[j];
        tie = tie && offer;
        uint32_t ri = i, rj[CAP];
#pragma unroll
        for (int j = 0; j < CAP; ++j) rj[j] = index[j];
        if (perm && tie) {
            ri = perm[i];
#pragma unroll
            for (int j = 0; j < CAP; ++j)
                if (d == d2[j]) rj[j] = reported(perm, index[j]);
        }
        bool before[CAP];  // monotone in j: the list is sorted
#pragma unroll
        for (int j = 0; j < CAP; ++j) before[j] = offer && (d < d2[j] || (d == d2[j] && ri < rj[j]));
#pragma unroll
        for (int j = CAP - 1; j >= 0; --j) {
            const bool shifted = j > 0 && before[j > 0 ? j - 1 : 0];
            const float dj = shifted ? d2[j > 0 ? j - 1 : 0] : d;
            const uint32_t ij = shifted ? index[j > 0 ? j - 1 : 0] : i;
            d2[j] = before[j] ? dj : d2[j];
            index[j] = before[j] ? ij : index[j];
        }
        float kth = kInf;
        uint32_t kth_index = kNoPrim;
#pragma unroll
        for (int j = 0; j < CAP; ++j) {  // (k is in an SGPR: a scalar compare and two selects per slot, no indexing)
            kth = static_cast<uint32_t>(j) + 1u == k ? d2[j] : kth;
            kth_index = static_cast<uint32_t>(j) + 1u == k ? index[j] : kth_index;
        }
        bound = kth_index != kNoPrim ? kth : max_d2;
    }
};

// A candidate is offered iff d2 <= bound (false for a NaN); the chain is entered only when some lane of the wave offers (accept_near of rvpt_query.hip)
template <int CAP>
__device__ __forceinline__ void offer_near(const uint32_t *perm, const float d2, const uint32_t i, const float max_d2, const uint32_t k, NearList<CAP> &h)
{
    const bool offer = d2 <= h.bound;
    if (ballot(offer) != 0) {
        asm volatile("" ::: "memory");  // keep this a (wave-uniform) branch
        h.insert(perm, offer, d2, i, max_d2, k);
    }
}

// A group's out fields: slot j's candidate recomputed from its row as store_point does, the miss quads from the first empty slot (empty slots come last).
// Slots at and past k are never stored; no in field of any record is.
template <int CAP>
__device__ __forceinline__ void store_points(float4 *records, const size_t group, const NearestPoint &q, const float4 *tris, const uint32_t *perm, const uint32_t k,
                                             const NearList<CAP> &h)
{
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (static_cast<uint32_t>(j) < k) store_point(records, group * k + static_cast<uint32_t>(j), q, tris, perm, h.index[j]);
}

}  // namespace

// LDS: [stack: lds_levels x 2 words x kBlock] — a slot is (box_d2 bits, node index), WalkStack<2> of rvpt_walk.h; the global part likewise.
__global__ __launch_bounds__(kBlock) void nearest_bvh2(const NearestArgs a)
{
    const WalkStack<2> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const uint32_t n_nodes = a.n_nodes, n_tris = a.n_tris;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;
        const bool live = r < a.n;
        const NearestPoint q = load_point(a.records, r, live);
        float best = __uint_as_float(q.max_bits);
        uint32_t best_i = kNoPrim, sp = 0, cur = 0;
        bool walking = q.valid && n_nodes > 0u;
        if (walking) walking = box_d2(q.p, a.nodes[0], a.nodes[1]) <= best;  // the root is a node like any other
        while (ballot(walking) != 0) {
            if (walking) {  // cur < n_nodes, and its box passed box_d2 <= best when it was chosen
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                if (count > 0) {
                    const uint32_t end = static_cast<uint32_t>(min(static_cast<uint64_t>(first) + count, static_cast<uint64_t>(n_tris)));  // (first >= n_tris: no triangle)
                    for (uint32_t i = first; i < end; ++i) accept(a.perm, closest_point_row(a.tris + 4 * static_cast<size_t>(i), q.p).d2, i, best, best_i);
                } else if (first < n_nodes && first + 1u < n_nodes) {  // both children inside the node buffer (first + 1 may wrap: then first fails)
                    const float4 *kids = a.nodes + 2u * static_cast<size_t>(first);
                    const float dl = box_d2(q.p, kids[0], kids[1]), dr = box_d2(q.p, kids[2], kids[3]);
                    const bool vl = dl <= best, vr = dr <= best;
                    const bool left_first = dl <= dr || !vr;
                    if (vl && vr) {
                        const float far_d = left_first ? dr : dl;
                        const uint32_t far_node = left_first ? first + 1u : first;
                        stack.push(sp, __float_as_uint(far_d), far_node);  // (the tree's height bounds the pushes of a root-to-leaf path)
                    }
                    if (vl || vr) {
                        cur = (vl && left_first) ? first : first + 1u;
                        pop = false;
                    }
                }
                if (pop) {
                    bool found = false;
                    while (sp > 0 && !found) {
                        uint32_t d_bits, node;
                        stack.pop(sp, d_bits, node);
                        if (__uint_as_float(d_bits) <= best && node < n_nodes) {  // best may have shrunk since the push
                            cur = node;
                            found = true;
                        }
                    }
                    walking = found;
                }
            }
        }
        if (live) store_point(a.records, r, q, a.tris, a.perm, best_i);
    }
}

// Brute force: a work-group answers 256 records and streams the vertex quads of the triangle rows through LDS in tiles of kNearestTileTris; every lane runs over
// each tile in index order.  (A brute-force context has no permutation, but nothing here relies on that.)
__global__ __launch_bounds__(kBlock) void nearest_brute(const NearestArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_rows[];
    const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = r < a.n;
    const NearestPoint q = load_point(a.records, r, live);
    float best = __uint_as_float(q.max_bits);
    uint32_t best_i = kNoPrim;
    if (__syncthreads_or(q.valid ? 1 : 0) != 0) {
        for (uint32_t base = 0; base < a.n_tris; base += kNearestTileTris) {
            const uint32_t count = min(kNearestTileTris, a.n_tris - base);
            for (uint32_t i = threadIdx.x; i < 3u * count; i += kBlock) lds_rows[i] = a.tris[4u * (static_cast<size_t>(base) + i / 3u) + i % 3u];
            __syncthreads();
            if (q.valid)
                for (uint32_t i = 0; i < count; ++i) accept(a.perm, closest_point_row(lds_rows + 3u * i, q.p).d2, base + i, best, best_i);
            __syncthreads();  // the barrier in front of the next tile's stores
        }
    }
    if (live) store_point(a.records, r, q, a.tris, a.perm, best_i);
}

// nearest_bvh2 with the list: the same walk, stack and claims over runs of 64 GROUPS
template <int CAP>
__global__ __launch_bounds__(kBlock) void nearest_bvh2_k(const NearestKArgs ka)
{
    const NearestArgs &a = ka.q;
    const uint32_t k = ka.k;
    const WalkStack<2> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const uint32_t n_nodes = a.n_nodes, n_tris = a.n_tris;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;  // the group
        const bool live = r < a.n;
        const NearestPoint q = load_point(a.records, r * k, live);  // record 0 of the group
        const float max_d2 = __uint_as_float(q.max_bits);
        NearList<CAP> h;
        h.reset(max_d2);
        uint32_t sp = 0, cur = 0;
        bool walking = q.valid && n_nodes > 0u;
        if (walking) walking = box_d2(q.p, a.nodes[0], a.nodes[1]) <= h.bound;  // the root is a node like any other
        while (ballot(walking) != 0) {
            if (walking) {  // cur < n_nodes, and its box passed box_d2 <= h.bound when it was chosen
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                if (count > 0) {
                    const uint32_t end = static_cast<uint32_t>(min(static_cast<uint64_t>(first) + count, static_cast<uint64_t>(n_tris)));  // (first >= n_tris: no triangle)
                    for (uint32_t i = first; i < end; ++i) offer_near(a.perm, closest_point_row(a.tris + 4 * static_cast<size_t>(i), q.p).d2, i, max_d2, k, h);
                } else if (first < n_nodes && first + 1u < n_nodes) {  // both children inside the node buffer (first + 1 may wrap: then first fails)
                    const float4 *kids = a.nodes + 2u * static_cast<size_t>(first);
                    const float dl = box_d2(q.p, kids[0], kids[1]), dr = box_d2(q.p, kids[2], kids[3]);
                    const bool vl = dl <= h.bound, vr = dr <= h.bound;
                    const bool left_first = dl <= dr || !vr;
                    if (vl && vr) {
                        const float far_d = left_first ? dr : dl;
                        const uint32_t far_node = left_first ? first + 1u : first;
                        stack.push(sp, __float_as_uint(far_d), far_node);  // (the tree's height bounds the pushes of a root-to-leaf path)
                    }
                    if (vl || vr) {
                        cur = (vl && left_first) ? first : first + 1u;
                        pop = false;
                    }
                }
                if (pop) {
                    bool found = false;
                    while (sp > 0 && !found) {
                        uint32_t d_bits, node;
                        stack.pop(sp, d_bits, node);
                        if (__uint_as_float(d_bits) <= h.bound && node < n_nodes) {  // bound may have shrunk since the push
                            cur = node;
                            found = true;
                        }
                    }
                    walking = found;
                }
            }
        }
        if (live) store_points(a.records, r, q, a.tris, a.perm, k, h);
    }
}

// nearest_brute with the list, over the same tiles
template <int CAP>
__global__ __launch_bounds__(kBlock) void nearest_brute_k(const NearestKArgs ka)
{
    const NearestArgs &a = ka.q;
    const uint32_t k = ka.k;
    extern __shared__ __attribute__((aligned(16))) float4 lds_rows[];
    const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;  // the group
    const bool live = r < a.n;
    const NearestPoint q = load_point(a.records, r * k, live);
    const float max_d2 = __uint_as_float(q.max_bits);
    NearList<CAP> h;
    h.reset(max_d2);
    if (__syncthreads_or(q.valid ? 1 : 0) != 0) {
        for (uint32_t base = 0; base < a.n_tris; base += kNearestTileTris) {
            const uint32_t count = min(kNearestTileTris, a.n_tris - base);
            for (uint32_t i = threadIdx.x; i < 3u * count; i += kBlock) lds_rows[i] = a.tris[4u * (static_cast<size_t>(base) + i / 3u) + i % 3u];
            __syncthreads();
            if (q.valid)
                for (uint32_t i = 0; i < count; ++i) offer_near(a.perm, closest_point_row(lds_rows + 3u * i, q.p).d2, base + i, max_d2, k, h);
            __syncthreads();  // the barrier in front of the next tile's stores
        }
    }
    if (live) store_points(a.records, r, q, a.tris, a.perm, k, h);
}

namespace {

using NearestKKernel = void (*)(NearestKArgs);

// the instance that answers k entries per point: the smallest list that holds them
NearestKKernel nearest_k_kernel(const bool brute, const uint32_t k)
{
    if (k <= 2u) return brute ? nearest_brute_k<2> : nearest_bvh2_k<2>;
    if (k <= 4u) return brute ? nearest_brute_k<4> : nearest_bvh2_k<4>;
    return brute ? nearest_brute_k<8> : nearest_bvh2_k<8>;
}

}  // namespace

hipError_t nearest_plan(const NearestScene &scene, const uint32_t n, const int num_cus, QueryPlan *plan, const uint32_t k)
{
    if (k == 0u || k > kNearestMaxK) return hipErrorInvalidValue;
    QueryPlan p{};
    if (scene.brute) {
        p.grid = std::max<uint32_t>(1u, static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlock - 1u) / kBlock));
        p.lds_bytes = static_cast<size_t>(kNearestTileTris) * 48u;
        *plan = p;
        return hipSuccess;
    }
    const uint32_t levels = std::max<uint32_t>(1u, scene.stack_levels);
    p.lds_levels = std::min(levels, kQueryLdsLevels);
    p.lds_bytes = static_cast<size_t>(p.lds_levels) * kBlock * 2u * sizeof(uint32_t);
    int per_cu = 0;
    const void *kernel = k > 1u ? reinterpret_cast<const void *>(nearest_k_kernel(false, k)) : reinterpret_cast<const void *>(nearest_bvh2);  // the instance that will run
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, p.lds_bytes);
    if (e != hipSuccess) return e;
    const uint64_t runs = (static_cast<uint64_t>(n) + 63u) / 64u;
    const uint64_t want = (runs + kBlock / 64u - 1u) / (kBlock / 64u);  // a work-group's four waves claim a run each
    p.grid = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(want, static_cast<uint64_t>(std::max(per_cu, 1)) * static_cast<uint64_t>(std::max(num_cus, 1)))));
    const size_t column_words = static_cast<size_t>(2u) * (levels - p.lds_levels) * kBlock;  // per work-group
    while (p.grid > 1u && column_words * p.grid * sizeof(uint32_t) > kQueryStackMaxBytes) p.grid = (p.grid + 1u) / 2u;
    p.stack_words = column_words * p.grid;
    *plan = p;
    return hipSuccess;
}

hipError_t nearest_launch(hipStream_t stream, const NearestScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n, const uint32_t k)
{
    if (k == 0u || k > kNearestMaxK) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    NearestArgs a{};
    a.tris = scene.tris, a.nodes = scene.nodes, a.perm = scene.perm;
    a.records = static_cast<float4 *>(records);
    a.n = n;
    a.n_runs = static_cast<uint32_t>((static_cast<uint64_t>(n) + 63u) / 64u);
    a.counter = scratch;
    a.stack_overflow = scratch + 64;
    a.n_tris = scene.n_tris, a.n_nodes = scene.n_nodes;
    a.stack_levels = std::max<uint32_t>(1u, scene.stack_levels);
    a.lds_levels = plan.lds_levels;
    if (k > 1u) {
        const NearestKArgs ka{a, k};
        if (!scene.brute) {
            const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(nearest_k_kernel(scene.brute, k), dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, ka);
        return hipGetLastError();
    }
    if (scene.brute) {
        hipLaunchKernelGGL(nearest_brute, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
        return hipGetLastError();
    }
    const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nearest_bvh2, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace rv
