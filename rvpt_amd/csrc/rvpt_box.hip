// rvpt_box.hip — box queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_BOX_OVERLAPS, RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k)): a group of k records comes in as a closed
// box and a first number, and goes out as the count of the triangles that meet the box and the 4k - 1 smallest of their numbers.
//
// THE ANSWER IS DEFINED WITHOUT A WALK (BOX OVERLAPS at rvpt_hip_read; rvpt_amd/scene.py: triangle_box_overlaps / box_overlaps state it in numpy): A is the set
// of stored triangles that pass triangle_meets_box() (rvpt_box.h: THE TEST) and whose reported number is >= prim_from; count = |A|, the slots hold the smallest
// numbers of A in ascending order, 0xFFFFFFFF from the first slot A does not fill.
//
// WHY PRUNING IS EXACT.  Step 1 of the test uses no arithmetic: it rejects iff on some axis all three vertices lie above hi or all three below lo.  Every box
// of every tree here contains the finite vertices under it (the builders and every refit take the min and max of them; a caller's loose boxes contain more).  So
// for a triangle that passes step 1 — which has only finite vertices, with on every axis one at or below hi and one at or above lo — node.lo <= hi and
// node.hi >= lo hold on every axis for every node above it: none of the six comparisons of box_apart() can reject an ancestor.  A walk that skips a node iff
// box_apart() holds therefore skips no triangle of A, and one it does not skip is decided by the test itself: the walk returns the definition's A on any tree,
// in any visiting order.  A node's side that is a NaN rejects nothing either.
//
// One box per lane.  box_bvh2<CAP> walks the BINARY nodes — the form every update keeps current — on the queries' persistent grid: waves claim runs of 64
// groups, the first stack levels per lane live in LDS and the rest in one global column per thread of the grid, as in nearest_bvh2, with ONE word per slot: there
// is no ordering between children and nothing to re-test at a pop.  There is no early exit.  A lane keeps `count` and the CAP smallest numbers, sorted, in VGPRs
// (CAP = 3, 7, 15: k = 1, 2, 4; k = 3 runs on the 15 and stores 11); the permutation word is loaded once per accepted triangle.  box_brute<CAP> streams the
// vertex rows through LDS in nearest_brute's tiles.  Only the out quads are stored.  An index read from the tree never becomes an address unchecked.  Each stored
// triangle is taken to lie under one leaf; a caller's tree that lists it under two may count it twice.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rvpt_device.h"
#include "rvpt_box.h"
#include "rvpt_walk.h"

namespace rv {

namespace {

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;

struct BoxArgs {
    const float4 *tris, *nodes;
    const uint32_t *perm;
    float4 *records;
    uint32_t n, n_runs;          // groups, runs of 64 groups
    uint32_t *counter;           // the next run to claim (0 at launch)
    uint32_t *stack_overflow;    // [stack_levels - lds_levels][threads of the grid]
    uint32_t n_tris, n_nodes, stack_levels, lds_levels;
    uint32_t k;                  // records per group, 1 .. kBoxMaxGroup (wave-uniform)
};

struct BoxRecord {
    BoxProbe q;
    uint32_t prim_from;
    bool valid;
};

__device__ __forceinline__ bool finite_(const float x) { return __builtin_fabsf(x) < kInf; }  // false for NaN and +-inf

// Record 0 of a group.  A box with a non-finite corner component, or with lo above hi on some axis, is answered before any walk; lo == hi is a box.
__device__ __forceinline__ BoxRecord load_box(const float4 *records, const size_t r, const bool live)
{
    const float4 a = live ? records[3 * r + 0] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 b = live ? records[3 * r + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
    BoxRecord g;
    g.q = box_probe(mk(a.x, a.y, a.z), mk(b.x, b.y, b.z));
    g.prim_from = __float_as_uint(a.w);
    g.valid = live && finite_(a.x) && finite_(a.y) && finite_(a.z) && finite_(b.x) && finite_(b.y) && finite_(b.z) && a.x <= b.x && a.y <= b.y && a.z <= b.z;
    return g;
}

// `count` and the CAP smallest reported numbers so far, ascending; an empty slot is kNoPrim, which no number is above, so empty slots come last.  Constant
// indices only, every loop unrolled: the list stays in VGPRs (NearList of rvpt_nearest.hip, with one word per slot and no ties to break: equal numbers — a
// triangle a caller's tree lists twice — sit side by side).
template <int CAP>
struct BoxList {
    uint32_t count;
    uint32_t prim[CAP];

    __device__ __forceinline__ void reset()
    {
        count = 0;
#pragma unroll
        for (int j = 0; j < CAP; ++j) prim[j] = kNoPrim;
    }
    // In front of the first entry above `number`, the rest one slot down, the last dropped.  From the last slot up, so that slot j - 1 is still the old one
    // when slot j takes it.
    __device__ __forceinline__ void insert(const bool offer, const uint32_t number)
    {
        count += offer ? 1u : 0u;
        bool before[CAP];  // monotone in j: the list is sorted
#pragma unroll
        for (int j = 0; j < CAP; ++j) before[j] = offer && number < prim[j];
#pragma unroll
        for (int j = CAP - 1; j >= 0; --j) {
            const bool shifted = j > 0 && before[j > 0 ? j - 1 : 0];
            const uint32_t pj = shifted ? prim[j > 0 ? j - 1 : 0] : number;
            prim[j] = before[j] ? pj : prim[j];
        }
    }
};

// One stored triangle against a lane's box: the test, then — for the lanes it accepts — the permutation word, the prim_from rule and the list
template <int CAP>
__device__ __forceinline__ void offer_triangle(const uint32_t *perm, const float4 *row, const uint32_t i, const bool asking, const BoxRecord &g, BoxList<CAP> &h)
{
    const float4 a = row[0], b = row[1], c = row[2];
    const bool meets = asking && triangle_meets_box(mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), g.q);
    if (ballot(meets) != 0) {
        asm volatile("" ::: "memory");  // keep this a (wave-uniform) branch
        uint32_t number = i;
        if (perm && meets) number = perm[i];
        h.insert(meets && number >= g.prim_from, number);
    }
}

// A group's out quads: (count, three numbers) in record 0, four more numbers in each follower.  Slots at and past 4k - 1 are never stored; no in quad is.
template <int CAP>
__device__ __forceinline__ void store_group(float4 *records, const size_t group, const uint32_t k, const BoxList<CAP> &h)
{
    uint32_t w[CAP + 1];
    w[0] = h.count;
#pragma unroll
    for (int j = 0; j < CAP; ++j) w[j + 1] = h.prim[j];
#pragma unroll
    for (int j = 0; j < (CAP + 1) / 4; ++j)
        if (static_cast<uint32_t>(j) < k)
            records[3 * (group * k + static_cast<uint32_t>(j)) + 2] =
                make_float4(__uint_as_float(w[4 * j]), __uint_as_float(w[4 * j + 1]), __uint_as_float(w[4 * j + 2]), __uint_as_float(w[4 * j + 3]));
}

// a binary node's box (bounds = {minx,maxx,miny,maxy,minz,maxz}: n0.zw = x, n1.xy = y, n1.zw = z) against the lane's
__device__ __forceinline__ bool node_apart(const BoxProbe &q, const float4 n0, const float4 n1)
{
    return box_apart(q, mk(n0.z, n1.x, n1.z), mk(n0.w, n1.y, n1.w));
}

}  // namespace

// LDS: [stack: lds_levels x kBlock words] — a slot is a node index, WalkStack<1> of rvpt_walk.h; the global part likewise.
template <int CAP>
__global__ __launch_bounds__(kBlock) void box_bvh2(const BoxArgs a)
{
    const uint32_t k = a.k;
    const WalkStack<1> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const uint32_t n_nodes = a.n_nodes, n_tris = a.n_tris;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;  // the group
        const bool live = r < a.n;
        const BoxRecord g = load_box(a.records, r * k, live);  // record 0 of the group
        BoxList<CAP> h;
        h.reset();
        uint32_t sp = 0, cur = 0;
        bool walking = g.valid && n_nodes > 0u;
        if (walking) walking = !node_apart(g.q, a.nodes[0], a.nodes[1]);  // the root is a node like any other
        while (ballot(walking) != 0) {
            if (walking) {  // cur < n_nodes, and its box was not apart when it was chosen
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                if (count > 0) {
                    const uint32_t end = static_cast<uint32_t>(min(static_cast<uint64_t>(first) + count, static_cast<uint64_t>(n_tris)));  // (first >= n_tris: no triangle)
                    for (uint32_t i = first; i < end; ++i) offer_triangle(a.perm, a.tris + 4 * static_cast<size_t>(i), i, true, g, h);
                } else if (first < n_nodes && first + 1u < n_nodes) {  // both children inside the node buffer (first + 1 may wrap: then first fails)
                    const float4 *kids = a.nodes + 2u * static_cast<size_t>(first);
                    const bool vl = !node_apart(g.q, kids[0], kids[1]), vr = !node_apart(g.q, kids[2], kids[3]);
                    if (vl && vr) stack.push(sp, first + 1u);  // (the tree's height bounds the pushes of a root-to-leaf path)
                    if (vl || vr) {
                        cur = vl ? first : first + 1u;
                        pop = false;
                    }
                }
                if (pop) {
                    bool found = false;
                    while (sp > 0 && !found) {
                        const uint32_t node = stack.pop(sp);
                        if (node < n_nodes) {
                            cur = node;
                            found = true;
                        }
                    }
                    walking = found;
                }
            }
        }
        if (live) store_group(a.records, r, k, h);
    }
}

// Brute force: a work-group answers 256 groups and streams the vertex quads of the triangle rows through LDS in tiles of kNearestTileTris; every lane runs over
// each tile in index order.  (A brute-force context has no permutation, but nothing here relies on that.)
template <int CAP>
__global__ __launch_bounds__(kBlock) void box_brute(const BoxArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_rows[];
    const uint32_t k = a.k;
    const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;  // the group
    const bool live = r < a.n;
    const BoxRecord g = load_box(a.records, r * k, live);
    BoxList<CAP> h;
    h.reset();
    if (__syncthreads_or(g.valid ? 1 : 0) != 0) {
        for (uint32_t base = 0; base < a.n_tris; base += kNearestTileTris) {
            const uint32_t count = min(kNearestTileTris, a.n_tris - base);
            for (uint32_t i = threadIdx.x; i < 3u * count; i += kBlock) lds_rows[i] = a.tris[4u * (static_cast<size_t>(base) + i / 3u) + i % 3u];
            __syncthreads();
            for (uint32_t i = 0; i < count; ++i) offer_triangle(a.perm, lds_rows + 3u * i, base + i, g.valid, g, h);  // (count is uniform: every lane of a wave is here)
            __syncthreads();  // the barrier in front of the next tile's stores
        }
    }
    if (live) store_group(a.records, r, k, h);
}

namespace {

using BoxKernel = void (*)(BoxArgs);

// the instance that answers groups of k records: the smallest list that holds their 4k - 1 numbers
BoxKernel box_kernel(const bool brute, const uint32_t k)
{
    if (k <= 1u) return brute ? box_brute<3> : box_bvh2<3>;
    if (k <= 2u) return brute ? box_brute<7> : box_bvh2<7>;
    return brute ? box_brute<15> : box_bvh2<15>;
}

}  // namespace

hipError_t box_plan(const NearestScene &scene, const uint32_t n, const int num_cus, QueryPlan *plan, const uint32_t k)
{
    if (k == 0u || k > kBoxMaxGroup) return hipErrorInvalidValue;
    QueryPlan p{};
    if (scene.brute) {
        p.grid = std::max<uint32_t>(1u, static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlock - 1u) / kBlock));
        p.lds_bytes = static_cast<size_t>(kNearestTileTris) * 48u;
        *plan = p;
        return hipSuccess;
    }
    const uint32_t levels = std::max<uint32_t>(1u, scene.stack_levels);
    p.lds_levels = std::min(levels, kQueryLdsLevels);
    p.lds_bytes = static_cast<size_t>(p.lds_levels) * kBlock * sizeof(uint32_t);
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(box_kernel(false, k)), kBlock, p.lds_bytes);  // the instance that will run
    if (e != hipSuccess) return e;
    const uint64_t runs = (static_cast<uint64_t>(n) + 63u) / 64u;
    const uint64_t want = (runs + kBlock / 64u - 1u) / (kBlock / 64u);  // a work-group's four waves claim a run each
    p.grid = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(want, static_cast<uint64_t>(std::max(per_cu, 1)) * static_cast<uint64_t>(std::max(num_cus, 1)))));
    const size_t column_words = static_cast<size_t>(levels - p.lds_levels) * kBlock;  // per work-group
    while (p.grid > 1u && column_words * p.grid * sizeof(uint32_t) > kQueryStackMaxBytes) p.grid = (p.grid + 1u) / 2u;
    p.stack_words = column_words * p.grid;
    *plan = p;
    return hipSuccess;
}

hipError_t box_launch(hipStream_t stream, const NearestScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n, const uint32_t k)
{
    if (k == 0u || k > kBoxMaxGroup) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    BoxArgs a{};
    a.tris = scene.tris, a.nodes = scene.nodes, a.perm = scene.perm;
    a.records = static_cast<float4 *>(records);
    a.n = n;
    a.n_runs = static_cast<uint32_t>((static_cast<uint64_t>(n) + 63u) / 64u);
    a.counter = scratch;
    a.stack_overflow = scratch + 64;
    a.n_tris = scene.n_tris, a.n_nodes = scene.n_nodes;
    a.stack_levels = std::max<uint32_t>(1u, scene.stack_levels);
    a.lds_levels = plan.lds_levels;
    a.k = k;
    if (!scene.brute) {
        const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(box_kernel(scene.brute, k), dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace rv
