// rvpt_sweep.hip — sphere sweeps (include/rvpt_hip.h: RVPT_HIP_FORMAT_SPHERE_SWEEPS): a record comes in as a sphere (org, radius) and a motion (dir, tmax) of its
// centre, and goes out as the time of its first contact with the mesh, the triangle, and the barycentric pair of the point of that triangle nearest to the
// centre at that time — the out quad of a ray query, which pipes into a surface read.
//
// THE ANSWER IS DEFINED WITHOUT A WALK (SPHERE SWEEPS at rvpt_hip_read; rvpt_amd/scene.py: sweep_sphere_triangles / sphere_sweeps state it in numpy): every
// stored triangle i gets a candidate (t_i, prim_i) or none from sweep_candidate() (rvpt_sweep.h: the own box's slab test, the seven features, the reported
// time), and the answer is the lexicographically smallest candidate.  binary32 with every product, sum, quotient and square root rounded on its own: this
// translation unit is compiled with -ffp-contract=off and without fast-math like every other, nothing here calls fma_(), the divisions are plain `/` and the
// square roots __builtin_sqrtf, which hipcc expands to the correctly rounded IEEE ones.
//
// WHY ANY WALK GIVES THAT ANSWER.  t_i = max(t_tri, t_in) with t_in the entry time of the centre's path into the triangle's OWN box inflated by r.  The box of
// every node above the triangle contains its (finite) vertices, lo - r and hi + r are monotone, and so is every operation of sweep_slab(): the node's slab
// test passes whenever the own box's does, with t_in(node) <= t_in(own) <= t_i IN FLOATS.  A walk that skips a node iff its slab test fails or t_in(node) >
// best (strict: at equality a smaller number may lie below) never skips a candidate that could win or tie: the visiting order is free.
//
// One record per lane.  sweep_bvh2 is nearest_bvh2's walk (rvpt_nearest.hip) over the BINARY nodes — the form every update keeps current — on the queries'
// persistent grid: waves claim runs of 64 records, the first stack levels per lane live in LDS and the rest in one global column per thread of the grid.  The
// child with the smaller t_in goes first, the other is stacked with its t_in and popped only while t_in <= best still holds.  sweep_brute streams the vertex rows
// through LDS in nearest_brute's tiles.  Only the out quad is stored.  An index read from the tree never becomes an address unchecked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rvpt_device.h"
#include "rvpt_sweep.h"
#include "rvpt_walk.h"

namespace rv {

namespace {

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;

struct SweepArgs {
    const float4 *tris, *nodes;
    const uint32_t *perm;
    float4 *records;
    uint32_t n, n_runs;          // records, runs of 64 records
    uint32_t *counter;           // the next run to claim (0 at launch)
    uint32_t *stack_overflow;    // [stack_levels - lds_levels][2][threads of the grid]
    uint32_t n_tris, n_nodes, stack_levels, lds_levels;
};

// A record's in quads and the bits of its tmax, which a miss gives back; a lane past the end gets an invalid record
__device__ __forceinline__ SweepProbe load_sweep(const float4 *records, const size_t r, const bool live, uint32_t &tmax_bits)
{
    const float4 a = live ? records[3 * r + 0] : make_float4(0.f, 0.f, 0.f, -1.f);
    const float4 b = live ? records[3 * r + 1] : make_float4(0.f, 0.f, 0.f, -1.f);
    tmax_bits = __float_as_uint(b.w);
    return sweep_probe(mk(a.x, a.y, a.z), a.w, mk(b.x, b.y, b.z), b.w);
}

__device__ __forceinline__ uint32_t reported(const uint32_t *perm, const uint32_t i) { return i == kNoPrim ? kNoPrim : (perm ? perm[i] : i); }

// One stored triangle against a lane's sweep: the own box, then — only where some lane of the wave passed it — the seven features, then (t, prim of i) against
// (best, prim of best_i), lexicographically.  The perm words are loaded only on a tie.
__device__ __forceinline__ void offer_triangle(const uint32_t *perm, const float4 *row, const uint32_t i, const bool asking, const SweepProbe &q, float &best, uint32_t &best_i)
{
    const float4 ra = row[0], rb = row[1], rc = row[2];
    const f3 a = mk(ra.x, ra.y, ra.z), b = mk(rb.x, rb.y, rb.z), c = mk(rc.x, rc.y, rc.z);
    float t_in;
    const bool passes = asking && sweep_own_box(q, a, b, c, t_in) && t_in <= best;  // (t >= t_in: a box entered after `best` holds no winner and no tie)
    if (ballot(passes) != 0) {
        asm volatile("" ::: "memory");  // keep this a (wave-uniform) branch
        float t;
        const bool has = sweep_reported(t_in, sweep_contact(q, a, b, c), t) && passes;
        if (has && t < best) {
            best = t;
            best_i = i;
        } else if (has && t == best) {
            if (reported(perm, i) < reported(perm, best_i)) best = t, best_i = i;  // (t too: it equals best, but a tmax of -0.0 must not stand for a contact at +0.0)
        }
    }
}

// A record's out quad.  The winner's pair is closest_point()'s for the centre at the reported time.
__device__ __forceinline__ void store_sweep(float4 *records, const size_t r, const SweepProbe &q, const float4 *tris, const uint32_t *perm, const uint32_t tmax_bits, const float best,
                                            const uint32_t best_i)
{
    float4 out = make_float4(__uint_as_float(tmax_bits), __uint_as_float(kNoPrim), 0.0f, 0.0f);
    if (best_i != kNoPrim) {
        const float4 *row = tris + 4 * static_cast<size_t>(best_i);
        const float4 ra = row[0], rb = row[1], rc = row[2];
        const Closest c = closest_point(mk(ra.x, ra.y, ra.z), mk(rb.x, rb.y, rb.z), mk(rc.x, rc.y, rc.z), q.p + q.d * best);
        out = make_float4(best, __uint_as_float(reported(perm, best_i)), c.u, c.v);
    }
    records[3 * r + 2] = out;
}

// a binary node's box (bounds = {minx,maxx,miny,maxy,minz,maxz}: n0.zw = x, n1.xy = y, n1.zw = z) against the lane's sweep
__device__ __forceinline__ bool node_slab(const SweepProbe &q, const float4 n0, const float4 n1, float &t_in)
{
    return sweep_slab(q, mk(n0.z, n1.x, n1.z), mk(n0.w, n1.y, n1.w), t_in);
}

}  // namespace

// LDS: [stack: lds_levels x 2 words x kBlock] — a slot is (t_in bits, node index), WalkStack<2> of rvpt_walk.h; the global part likewise.
__global__ __launch_bounds__(kBlock) void sweep_bvh2(const SweepArgs a)
{
    const WalkStack<2> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const uint32_t n_nodes = a.n_nodes, n_tris = a.n_tris;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;
        const bool live = r < a.n;
        uint32_t tmax_bits;
        const SweepProbe q = load_sweep(a.records, r, live, tmax_bits);
        float best = q.tmax;
        uint32_t best_i = kNoPrim, sp = 0, cur = 0;
        bool walking = q.valid && n_nodes > 0u;
        if (walking) {  // the root is a node like any other
            float t_root;
            walking = node_slab(q, a.nodes[0], a.nodes[1], t_root) && t_root <= best;
        }
        while (ballot(walking) != 0) {
            if (walking) {  // cur < n_nodes, and its box passed the slab test with t_in <= best when it was chosen
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                if (count > 0) {
                    const uint32_t end = static_cast<uint32_t>(min(static_cast<uint64_t>(first) + count, static_cast<uint64_t>(n_tris)));  // (first >= n_tris: no triangle)
                    for (uint32_t i = first; i < end; ++i) offer_triangle(a.perm, a.tris + 4 * static_cast<size_t>(i), i, true, q, best, best_i);
                } else if (first < n_nodes && first + 1u < n_nodes) {  // both children inside the node buffer (first + 1 may wrap: then first fails)
                    const float4 *kids = a.nodes + 2u * static_cast<size_t>(first);
                    float tl, tr;
                    const bool vl = node_slab(q, kids[0], kids[1], tl) && tl <= best, vr = node_slab(q, kids[2], kids[3], tr) && tr <= best;
                    const bool left_first = tl <= tr || !vr;
                    if (vl && vr) {
                        const float far_t = left_first ? tr : tl;
                        const uint32_t far_node = left_first ? first + 1u : first;
                        stack.push(sp, __float_as_uint(far_t), far_node);  // (the tree's height bounds the pushes of a root-to-leaf path)
                    }
                    if (vl || vr) {
                        cur = (vl && left_first) ? first : first + 1u;
                        pop = false;
                    }
                }
                if (pop) {
                    bool found = false;
                    while (sp > 0 && !found) {
                        uint32_t t_bits, node;
                        stack.pop(sp, t_bits, node);
                        if (__uint_as_float(t_bits) <= best && node < n_nodes) {  // best may have shrunk since the push
                            cur = node;
                            found = true;
                        }
                    }
                    walking = found;
                }
            }
        }
        if (live) store_sweep(a.records, r, q, a.tris, a.perm, tmax_bits, best, best_i);
    }
}

// Brute force: a work-group answers 256 records and streams the vertex quads of the triangle rows through LDS in tiles of kNearestTileTris; every lane runs over
// each tile in index order.  (A brute-force context has no permutation, but nothing here relies on that.)
__global__ __launch_bounds__(kBlock) void sweep_brute(const SweepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_rows[];
    const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = r < a.n;
    uint32_t tmax_bits;
    const SweepProbe q = load_sweep(a.records, r, live, tmax_bits);
    float best = q.tmax;
    uint32_t best_i = kNoPrim;
    if (__syncthreads_or(q.valid ? 1 : 0) != 0) {
        for (uint32_t base = 0; base < a.n_tris; base += kNearestTileTris) {
            const uint32_t count = min(kNearestTileTris, a.n_tris - base);
            for (uint32_t i = threadIdx.x; i < 3u * count; i += kBlock) lds_rows[i] = a.tris[4u * (static_cast<size_t>(base) + i / 3u) + i % 3u];
            __syncthreads();
            for (uint32_t i = 0; i < count; ++i) offer_triangle(a.perm, lds_rows + 3u * i, base + i, q.valid, q, best, best_i);  // (count is uniform: every lane of a wave is here)
            __syncthreads();  // the barrier in front of the next tile's stores
        }
    }
    if (live) store_sweep(a.records, r, q, a.tris, a.perm, tmax_bits, best, best_i);
}

hipError_t sweep_plan(const NearestScene &scene, const uint32_t n, const int num_cus, QueryPlan *plan)
{
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
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(sweep_bvh2), kBlock, p.lds_bytes);  // the kernel that will run
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

hipError_t sweep_launch(hipStream_t stream, const NearestScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n)
{
    if (n == 0) return hipSuccess;
    SweepArgs a{};
    a.tris = scene.tris, a.nodes = scene.nodes, a.perm = scene.perm;
    a.records = static_cast<float4 *>(records);
    a.n = n;
    a.n_runs = static_cast<uint32_t>((static_cast<uint64_t>(n) + 63u) / 64u);
    a.counter = scratch;
    a.stack_overflow = scratch + 64;
    a.n_tris = scene.n_tris, a.n_nodes = scene.n_nodes;
    a.stack_levels = std::max<uint32_t>(1u, scene.stack_levels);
    a.lds_levels = plan.lds_levels;
    if (scene.brute) {
        hipLaunchKernelGGL(sweep_brute, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
        return hipGetLastError();
    }
    const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sweep_bvh2, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace rv
