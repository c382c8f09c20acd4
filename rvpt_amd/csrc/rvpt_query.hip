// rvpt_query.hip — ray queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_RAY_HITS): a record comes in as a ray and goes out as a hit, in place.
//
// The walks are the frame kernels' with the path tracer taken out: the same slab test, the same triangle test, the same order (rvpt_device.h), so a query's
// answer is the closest_t / hit pair a frame's segment along that ray would shade — the reference's intersect_bvh (intersection.glsl:361-413: left child first,
// the interval shrinking with every accept) on BVH contexts, triangles 0 .. n-1 in stored order on brute-force contexts.  What a query adds: the interval starts
// at the record's tmax instead of +inf; a record with the any-hit bit stops at the FIRST triangle that order accepts; u and v of the accepting test go out.
//
// One ray per lane.  The tree walks run on a PERSISTENT grid sized from occupancy whose waves claim runs of 64 consecutive records: the part of the traversal
// stack that does not fit LDS is one global column per thread of the grid and level, bounded by the grid and not by the number of rays.  No camera packets: a
// caller's rays have no common origin.  A record is three float4; only the third (the out fields) is stored.
//
// THREE WALKS (walk_bvh4, walk_bvh2, walk_brute), each written once over a GATHERER, the per-lane state that takes what the walk finds:
//   Closest      — RAY_HITS as above: `closest` and `hit`; the interval ends at closest.
//   Nearest<CAP> — K-NEAREST RAY QUERIES (RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k)): `closest` replaced by `bound`, the t of the k-th entry of a sorted list of hits
//                  a lane keeps in registers (the record's tmax until the list is full; an any-hit lane's bound stays tmax and its list is in the order of
//                  acceptance).  n and n_runs count GROUPS of k records, one ray each.
//   Crossings    — RAY CROSSINGS (RVPT_HIP_FORMAT_RAY_CROSSINGS): reduced instead of listed.  The interval is (0, tmax) from start to end, so the set of
//                  accepted tests is that of an any-hit k-nearest walk with no limit on k and does not depend on the visiting order; a lane keeps two counts
//                  and the smallest and largest accepted t, and never leaves its walk early.
// No gatherer ever grows its interval, which is all the wide walk's equivalence with the binary one rests on.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rvpt_device.h"
#include "rvpt_query.h"
#include "rvpt_walk.h"

namespace rv {

namespace {

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;
constexpr uint32_t kRayAnyHit = 0x1u;  // RVPT_HIP_RAY_ANY_HIT
constexpr float kFltMax = 3.402823466e+38f;

struct QueryArgs {
    const float4 *prep, *nodes, *wide;
    const uint32_t *perm;
    float4 *records;
    uint32_t n, n_runs;          // rays, runs of 64 rays
    uint32_t *counter;           // the next run to claim (0 at launch)
    uint32_t *stack_overflow;    // [stack_levels - lds_levels][2][threads of the grid]
    uint32_t n_tris, head_shift, stack_levels, lds_levels, top_nodes;
};

struct QueryRay {
    f3 o, d;
    uint32_t tmax_bits;
    bool any, valid;
};

__device__ __forceinline__ bool finite_(const float x) { return __builtin_fabsf(x) < kInf; }  // false for NaN and +-inf

// A record's in fields.  A ray with a non-finite component is a miss before any walk; so is a tmax that is NaN, zero or negative (the interval (0, tmax) is empty).
__device__ __forceinline__ QueryRay load_ray(const float4 *records, const size_t r, const bool live)
{
    QueryRay q;
    const float4 a = live ? records[3 * r + 0] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 b = live ? records[3 * r + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
    q.o = mk(a.x, a.y, a.z);
    q.d = mk(b.x, b.y, b.z);
    q.tmax_bits = __float_as_uint(a.w);
    q.any = (__float_as_uint(b.w) & kRayAnyHit) != 0u;
    q.valid = live && finite_(a.x) && finite_(a.y) && finite_(a.z) && finite_(b.x) && finite_(b.y) && finite_(b.z) && a.w > 0.0f;
    return q;
}

// A record's out fields.  u and v are recomputed for the winning triangle with test_triangle's own expression (the same operations on the same operands: the
// same bits the accepting test had), which is cheaper than carrying two more registers through the walk.
__device__ __forceinline__ void store_hit(float4 *records, const size_t r, const QueryRay &q, const float4 *prep, const uint32_t *perm, const float closest,
                                          const uint32_t hit)
{
    float4 out = make_float4(__uint_as_float(q.tmax_bits), __uint_as_float(kNoPrim), 0.0f, 0.0f);
    if (hit != kNoPrim) {
        const v4f *tp = reinterpret_cast<const v4f *>(prep) + 4 * static_cast<size_t>(hit);
        const TriangleUV t = test_triangle_uv(unpack(tp[0], tp[1], tp[2], tp[3]), q.o, q.d);
        out = make_float4(closest, __uint_as_float(perm ? perm[hit] : hit), t.u, t.v);
    }
    records[3 * r + 2] = out;
}

// A GATHERER holds a lane's answer while its ray walks.  Args: the kernel's argument, QueryArgs and what the form adds to them.  kLeavesEarly: a lane can be
// finished before its walk is (an any-hit ray that is served).  stride(): records per ray.  bound(): the end of the interval the slab tests and the pops compare
// against.  leaf(): a leaf's triangles in index order, true when the ray is finished.  tile(): one open test of a brute-force tile, `active` masking the accept
// and cleared when the ray is finished.  store(): the out fields of the ray whose first record is r.

struct ClosestArgs {
    QueryArgs q;
};
struct Closest {
    using Args = ClosestArgs;
    static constexpr bool kLeavesEarly = true;
    float closest;
    uint32_t hit;

    __device__ __forceinline__ static uint32_t stride(const Args &) { return 1u; }
    __device__ __forceinline__ void reset(const Args &, const QueryRay &q) { closest = __uint_as_float(q.tmax_bits), hit = kNoPrim; }
    __device__ __forceinline__ float bound() const { return closest; }
    // an any-hit ray stops at the first accept
    __device__ __forceinline__ bool leaf(const Args &, const v4f *prep, const uint32_t first, const uint32_t count, const QueryRay &q)
    {
        for (uint32_t i = first; i < first + count; ++i) {
            const v4f *tp = prep + 4 * static_cast<size_t>(i);
            test_triangle(unpack(tp[0], tp[1], tp[2], tp[3]), q.o, q.d, i, closest, hit);
            if (q.any && hit != kNoPrim) return true;
        }
        return false;
    }
    // accept_hit (rvpt_device.h) with the query's rider: an any-hit lane leaves after its first accept
    __device__ __forceinline__ void tile(const Args &, const OpenTest r, const uint32_t index, const QueryRay &q, bool &active)
    {
        const bool accept = (r.m > 0.0f) & (r.s < 1.0f) & (r.tt < closest) & active;
        if (ballot(accept) != 0) {
            closest = accept ? r.tt : closest;
            hit = accept ? index : hit;
            active = active && !(accept && q.any);
        }
    }
    __device__ __forceinline__ void store(const Args &a, const size_t r, const QueryRay &q) const { store_hit(a.q.records, r, q, a.q.prep, a.q.perm, closest, hit); }
};

struct NearArgs {
    QueryArgs q;
    uint32_t k;  // hits per ray, 2 .. CAP (wave-uniform)
};
// CAP slots, t and the stored index of each, sorted by t (any hit: by acceptance); an empty slot is (+inf, kNoPrim) and empty slots come last.  An accepted
// t is below bound <= tmax, hence finite: no held hit compares above FLT_MAX, every empty slot does.  Slots at and past k fill like the others; nothing reads them.
// Constant indices only, every loop unrolled: the list stays in VGPRs.
template <int CAP>
struct Nearest {
    using Args = NearArgs;
    static constexpr bool kLeavesEarly = true;
    float t[CAP];
    uint32_t index[CAP];
    float bound_;  // the interval's end: tmax, or the k-th t once a closest-mode list holds k
    bool full;     // slot k - 1 is taken (an any-hit lane is finished)

    __device__ __forceinline__ static uint32_t stride(const Args &a) { return a.k; }
    __device__ __forceinline__ void reset(const Args &, const QueryRay &q)
    {
#pragma unroll
        for (int j = 0; j < CAP; ++j) t[j] = kInf, index[j] = kNoPrim;
        bound_ = __uint_as_float(q.tmax_bits);
        full = false;
    }
    __device__ __forceinline__ float bound() const { return bound_; }
    // Behind every entry whose t is <= tt (any hit: behind every entry), the rest one slot down, the last dropped.  From the last slot up, so that slot j - 1
    // is still the old one when slot j takes it.
    __device__ __forceinline__ void insert(const bool accept, const float tt, const uint32_t i, const bool any, const float tmax, const uint32_t k)
    {
        const float key = accept ? (any ? kFltMax : tt) : kInf;  // (no slot is above +inf: a lane that does not accept keeps its list)
#pragma unroll
        for (int j = CAP - 1; j >= 0; --j) {
            const bool here = t[j] > key;
            const bool shifted = j > 0 && t[j > 0 ? j - 1 : 0] > key;
            const float tj = shifted ? t[j > 0 ? j - 1 : 0] : tt;
            const uint32_t ij = shifted ? index[j > 0 ? j - 1 : 0] : i;
            t[j] = here ? tj : t[j];
            index[j] = here ? ij : index[j];
        }
        float kth = kInf;
        uint32_t kth_index = kNoPrim;
#pragma unroll
        // the k-th entry, over all CAP slots on every entry.  In closest mode slots at and past k may hold hits too (entries pushed down past the k-th): they are
        // at or above bound, deliberately never read, and never stored
        for (int j = 0; j < CAP; ++j) {  // (k is in an SGPR: a scalar compare and two selects per slot, no indexing)
            kth = static_cast<uint32_t>(j) + 1u == k ? t[j] : kth;
            kth_index = static_cast<uint32_t>(j) + 1u == k ? index[j] : kth_index;
        }
        full = kth_index != kNoPrim;
        bound_ = full && !any ? kth : tmax;
    }
    // the chain is entered only when some lane accepts
    __device__ __forceinline__ void offer(const bool accept, const float tt, const uint32_t i, const QueryRay &q, const uint32_t k)
    {
        if (ballot(accept) != 0) {
            asm volatile("" ::: "memory");  // keep this a (wave-uniform) branch, as accept_hit does
            insert(accept, tt, i, q.any, __uint_as_float(q.tmax_bits), k);
        }
    }
    // test_triangle's test against (0, bound); true when an any-hit ray holds its k
    __device__ __forceinline__ bool leaf(const Args &a, const v4f *prep, const uint32_t first, const uint32_t count, const QueryRay &q)
    {
        for (uint32_t i = first; i < first + count; ++i) {
            const v4f *tp = prep + 4 * static_cast<size_t>(i);
            const TriangleUV r = test_triangle_uv(unpack(tp[0], tp[1], tp[2], tp[3]), q.o, q.d);
            offer((0.0f < r.tt) & (r.tt < bound_) & (0.0f < r.u) & (0.0f < r.v) & (r.u + r.v < 1.0f), r.tt, i, q, a.k);
            if (q.any && full) return true;
        }
        return false;
    }
    __device__ __forceinline__ void tile(const Args &a, const OpenTest r, const uint32_t i, const QueryRay &q, bool &active)
    {
        offer((r.m > 0.0f) & (r.s < 1.0f) & (r.tt < bound_) & active, r.tt, i, q, a.k);
        active = active && !(q.any && full);
    }
    // A group's k out quads: slot j's hit with u and v recomputed as store_hit does, the miss quad for an empty slot.  Only the third float4 of a record is
    // stored, the followers' included.
    __device__ __forceinline__ void store(const Args &a, const size_t r, const QueryRay &q) const
    {
#pragma unroll
        for (int j = 0; j < CAP; ++j)
            if (static_cast<uint32_t>(j) < a.k) store_hit(a.q.records, r + static_cast<uint32_t>(j), q, a.q.prep, a.q.perm, t[j], index[j]);
    }
};

struct CrossArgs {
    QueryArgs q;
    const float4 *unit_n;  // n_tris: (normalize(n), 0) by stored index, as SURFACE POINTS returns it
};
struct Crossings {
    using Args = CrossArgs;
    static constexpr bool kLeavesEarly = false;
    uint32_t front, back;
    float t_near, t_far;  // +inf and +0 while nothing is accepted: an accepted t is in (0, tmax), finite and positive
    float tmax;

    __device__ __forceinline__ static uint32_t stride(const Args &) { return 1u; }
    __device__ __forceinline__ void reset(const Args &, const QueryRay &q) { front = 0u, back = 0u, t_near = kInf, t_far = 0.0f, tmax = __uint_as_float(q.tmax_bits); }
    __device__ __forceinline__ float bound() const { return tmax; }
    // An accepted test counts by its facing: s = (d.x n.x + d.y n.y) + d.z n.z, every operation rounded on its own; FRONT iff s < 0, everything else (s NaN
    // included) BACK.  The normal is gathered only by the lanes that accept, and only when some lane does.
    __device__ __forceinline__ void count(const bool accept, const float tt, const uint32_t i, const f3 d, const float4 *unit_n)
    {
        if (ballot(accept) != 0) {
            asm volatile("" ::: "memory");  // keep this a (wave-uniform) branch, as accept_hit does
            if (accept) {
                const float4 un = unit_n[i];
                const float s = __fadd_rn(__fadd_rn(__fmul_rn(d.x, un.x), __fmul_rn(d.y, un.y)), __fmul_rn(d.z, un.z));
                const bool is_front = s < 0.0f;
                front += is_front ? 1u : 0u;
                back += is_front ? 0u : 1u;
                t_near = __builtin_fminf(t_near, tt);
                t_far = __builtin_fmaxf(t_far, tt);
            }
        }
    }
    // every triangle of the leaf, no early return
    __device__ __forceinline__ bool leaf(const Args &a, const v4f *prep, const uint32_t first, const uint32_t n, const QueryRay &q)
    {
        for (uint32_t i = first; i < first + n; ++i) {
            const v4f *tp = prep + 4 * static_cast<size_t>(i);
            const TriangleUV r = test_triangle_uv(unpack(tp[0], tp[1], tp[2], tp[3]), q.o, q.d);
            count((0.0f < r.tt) & (r.tt < tmax) & (0.0f < r.u) & (0.0f < r.v) & (r.u + r.v < 1.0f), r.tt, i, q.d, a.unit_n);
        }
        return false;
    }
    __device__ __forceinline__ void tile(const Args &a, const OpenTest r, const uint32_t i, const QueryRay &q, const bool &active)  // (`active`: the ray is valid)
    {
        count((r.m > 0.0f) & (r.s < 1.0f) & (r.tt < tmax) & active, r.tt, i, q.d, a.unit_n);
    }
    // the counts, t_near and t_far; with nothing accepted (0, 0, the bits of tmax as given, +0)
    __device__ __forceinline__ void store(const Args &a, const size_t r, const QueryRay &q) const
    {
        const bool none = (front | back) == 0u;
        a.q.records[3 * r + 2] = make_float4(__uint_as_float(front), __uint_as_float(back), none ? __uint_as_float(q.tmax_bits) : t_near, t_far);
    }
};

}  // namespace

// The 4-wide walk of rvpt_walk.h (its order, its stack slots and its LDS layout are stated there) over the runs a wave claims
template <class G>
__global__ __launch_bounds__(kBlock) void walk_bvh4(const typename G::Args ga)
{
    const QueryArgs &a = ga.q;
    const WideTree tree(a.lds_levels, a.nodes, a.wide, a.top_nodes, a.head_shift);
    const WalkStack<2> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t ray = static_cast<size_t>(run) * 64u + lane;
        const bool live = ray < a.n;
        const size_t r = ray * G::stride(ga);  // the ray's first record
        const QueryRay q = load_ray(a.records, r, live);
        G g;
        g.reset(ga, q);
        uint32_t sp = 0;
        WideAt at;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        {
            float entry;  // the root is a node like any other: its own box first (intersection.glsl:369-380)
            walking = walking && slab_entry(q.o, inv, tree.lds_root[0], tree.lds_root[1], g.bound(), entry);
        }
        while (ballot(walking) != 0) {  // (a lane that is finished has left; the loop ends for the wave when none walks)
            bool need_pop = false;
            if (walking && at.leaf_count == 0) wide_step(tree, q.o, inv, g.bound(), stack, sp, at, need_pop);
            if (walking && at.leaf_count > 0) {
                if (g.leaf(ga, prep, at.leaf_first, at.leaf_count, q)) walking = false;
                at.leaf_count = 0;
                need_pop = true;
            }
            if (walking && need_pop) walking = wide_pop(tree, g.bound(), stack, sp, at);
        }
        if (live) g.store(ga, r, q);
    }
}

// intersect_bvh as the reference writes it, over the binary nodes (children of an inner node at first, first + 1): pop a node, test its box against the interval
// of that moment, a leaf's triangles in order, an inner node's right child stacked and its left child next.  One word per stack slot (the node index): the
// tree's height bounds the pushes of a root-to-leaf path.
template <class G>
__global__ __launch_bounds__(kBlock) void walk_bvh2(const typename G::Args ga)
{
    const QueryArgs &a = ga.q;
    const WalkStack<1> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t ray = static_cast<size_t>(run) * 64u + lane;
        const bool live = ray < a.n;
        const size_t r = ray * G::stride(ga);  // the ray's first record
        const QueryRay q = load_ray(a.records, r, live);
        G g;
        g.reset(ga, q);
        uint32_t sp = 0, cur = 0;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        while (ballot(walking) != 0) {
            if (walking) {
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)], n1 = a.nodes[2u * static_cast<size_t>(cur) + 1u];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                float entry;
                if (slab_entry(q.o, inv, n0, n1, g.bound(), entry)) {
                    if (count > 0) {
                        if (g.leaf(ga, prep, first, count, q)) walking = false;
                    } else {
                        stack.push(sp, first + 1u);
                        cur = first;
                        pop = false;
                    }
                }
                if ((walking || !G::kLeavesEarly) && pop) {
                    if (sp == 0) {
                        walking = false;
                    } else {
                        cur = stack.pop(sp);
                    }
                }
            }
        }
        if (live) g.store(ga, r, q);
    }
}

// Brute force: a work-group answers 256 rays and streams the prepared triangles through LDS in tiles of kQueryTileTris; every lane runs over each tile in
// index order.  Where lanes can leave early the loop ends for the work-group when no lane is left (every ray invalid, or every any-hit ray served); where they
// cannot, a work-group runs over every tile unless none of its rays is valid.
template <class G>
__global__ __launch_bounds__(kBlock) void walk_brute(const typename G::Args ga)
{
    const QueryArgs &a = ga.q;
    extern __shared__ __attribute__((aligned(16))) float4 lds_tile[];
    const size_t ray = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = ray < a.n;
    const size_t r = ray * G::stride(ga);  // the ray's first record
    const QueryRay q = load_ray(a.records, r, live);
    G g;
    g.reset(ga, q);
    bool active = q.valid;
    auto accept = [&](const OpenTest t, const uint32_t index) { g.tile(ga, t, index, q, active); };
    if (G::kLeavesEarly) {
        for (uint32_t base = 0; base < a.n_tris; base += kQueryTileTris) {
            const uint32_t count = min(kQueryTileTris, a.n_tris - base);
            for (uint32_t i = threadIdx.x; i < 4u * count; i += kBlock) lds_tile[i] = a.prep[4u * static_cast<size_t>(base) + i];
            __syncthreads();
            if (ballot(active) != 0) tile_run(reinterpret_cast<const v4f *>(lds_tile), base, count, q.o, q.d, accept);
            if (__syncthreads_or(active ? 1 : 0) == 0) break;  // (also the barrier in front of the next tile's stores)
        }
    } else if (__syncthreads_or(active ? 1 : 0) != 0) {
        for (uint32_t base = 0; base < a.n_tris; base += kQueryTileTris) {
            const uint32_t count = min(kQueryTileTris, a.n_tris - base);
            if (base != 0) __syncthreads();  // the last tile has been read by every wave
            for (uint32_t i = threadIdx.x; i < 4u * count; i += kBlock) lds_tile[i] = a.prep[4u * static_cast<size_t>(base) + i];
            __syncthreads();
            if (ballot(active) != 0) tile_run(reinterpret_cast<const v4f *>(lds_tile), base, count, q.o, q.d, accept);
        }
    }
    if (live) g.store(ga, r, q);
}

namespace {

template <class G>
const void *walk_of(const QueryKind kind)
{
    if (kind == QueryKind::Brute) return reinterpret_cast<const void *>(walk_brute<G>);
    return kind == QueryKind::Wide ? reinterpret_cast<const void *>(walk_bvh4<G>) : reinterpret_cast<const void *>(walk_bvh2<G>);
}

// The instance a launch runs; a k-nearest one is the smallest that holds k (2, 4 or 8 slots)
const void *kernel_for(const QueryForm form, const QueryKind kind, const uint32_t k)
{
    if (form == QueryForm::Crossings) return walk_of<Crossings>(kind);
    if (k <= 1u) return walk_of<Closest>(kind);  // k = 1 is format 2 itself
    return k <= 2u ? walk_of<Nearest<2>>(kind) : (k <= 4u ? walk_of<Nearest<4>>(kind) : walk_of<Nearest<8>>(kind));
}

}  // namespace

hipError_t query_plan(const QueryScene &scene, const QueryForm form, const uint32_t n, const int num_cus, QueryPlan *plan, const uint32_t k)
{
    QueryPlan p{};
    if (scene.kind == QueryKind::Brute) {
        p.grid = std::max<uint32_t>(1u, static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlock - 1u) / kBlock));
        p.lds_bytes = static_cast<size_t>(kQueryTileTris) * 64u;
        *plan = p;
        return hipSuccess;
    }
    const uint32_t levels = std::max<uint32_t>(1u, scene.stack_levels);
    p.lds_levels = std::min(levels, kQueryLdsLevels);
    p.top_nodes = scene.kind == QueryKind::Wide ? std::min(scene.n_wide, kQueryTopNodes) : 0u;
    p.lds_bytes = static_cast<size_t>(p.lds_levels) * kBlock * 2u * sizeof(uint32_t) + 2u * sizeof(float4) + static_cast<size_t>(p.top_nodes) * 128u;
    int per_cu = 0;
    // (the occupancy of the instance that is launched: a k-nearest instance holds its list in registers and may fit fewer waves)
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_for(form, scene.kind, k), kBlock, p.lds_bytes);
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

hipError_t query_launch(hipStream_t stream, const QueryScene &scene, const QueryForm form, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n,
                        const uint32_t k)
{
    if (n == 0) return hipSuccess;
    const bool crossings = form == QueryForm::Crossings;
    if (k == 0 || k > kQueryMaxHits || (crossings && k != 1u)) return hipErrorInvalidValue;
    if (crossings && scene.n_tris > 0 && !scene.unit_n) return hipErrorInvalidValue;
    ClosestArgs ca{};
    QueryArgs &a = ca.q;
    a.prep = scene.prep, a.nodes = scene.nodes, a.wide = scene.wide, a.perm = scene.perm;
    a.records = static_cast<float4 *>(records);
    a.n = n;
    a.n_runs = static_cast<uint32_t>((static_cast<uint64_t>(n) + 63u) / 64u);
    a.counter = scratch;
    a.stack_overflow = scratch + 64;
    a.n_tris = scene.n_tris, a.head_shift = scene.head_shift;
    a.stack_levels = std::max<uint32_t>(1u, scene.stack_levels);
    a.lds_levels = plan.lds_levels, a.top_nodes = plan.top_nodes;
    NearArgs na{a, k};
    CrossArgs xa{a, scene.unit_n};
    if (scene.kind != QueryKind::Brute) {
        const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    void *kernel_args[] = {crossings ? static_cast<void *>(&xa) : (k > 1u ? static_cast<void *>(&na) : static_cast<void *>(&ca))};  // the Args of kernel_for's gatherer
    return hipLaunchKernel(kernel_for(form, scene.kind, k), dim3(plan.grid), dim3(kBlock), kernel_args, plan.lds_bytes, stream);
}

}  // namespace rv
