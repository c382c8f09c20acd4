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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rvpt_device.h"
#include "rvpt_query.h"

namespace rv {

namespace {

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;
constexpr uint32_t kRayAnyHit = 0x1u;  // RVPT_HIP_RAY_ANY_HIT
constexpr float kFltMax = 3.402823466e+38f;

struct QueryArgs {
    const float4 *prep, *nodes, *wide;
    const uint32_t *perm;
    float4 *records;
    uint32_t n, n_runs;          // records, runs of 64 records
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
        const PrepTri t = unpack(tp[0], tp[1], tp[2], tp[3]);
        const float tt = div_dots(dot(t.v0 - q.o, t.n), dot(q.d, t.n));
        const f3 p0 = fma3(q.d, tt, q.o) - t.v0;
        const float b0 = dot(p0, t.e0);
        const float b1 = dot(p0, t.e1);
        const float u = t.inv_det * fma_(t.a01, b1, t.a00 * b0);
        const float v = t.inv_det * fma_(t.a11, b1, t.a01 * b0);
        out = make_float4(closest, __uint_as_float(perm ? perm[hit] : hit), u, v);
    }
    records[3 * r + 2] = out;
}

// A leaf's triangles in index order; an any-hit ray stops at the first accept (returns true: the ray is finished)
__device__ __forceinline__ bool test_leaf(const v4f *prep, const uint32_t first, const uint32_t count, const QueryRay &q, float &closest, uint32_t &hit)
{
    for (uint32_t i = first; i < first + count; ++i) {
        const v4f *tp = prep + 4 * static_cast<size_t>(i);
        test_triangle(unpack(tp[0], tp[1], tp[2], tp[3]), q.o, q.d, i, closest, hit);
        if (q.any && hit != kNoPrim) return true;
    }
    return false;
}

// intersect_run<4> (rvpt_device.h) with the query's rider: `active` masks the accept, and an any-hit lane leaves after its first one
__device__ __forceinline__ void accept_query(const OpenTest r, const uint32_t index, const bool any, float &closest, uint32_t &hit, bool &active)
{
    const bool accept = (r.m > 0.0f) & (r.s < 1.0f) & (r.tt < closest) & active;
    if (ballot(accept) != 0) {
        closest = accept ? r.tt : closest;
        hit = accept ? index : hit;
        active = active && !(accept && any);
    }
}
__device__ __forceinline__ void query_run(const v4f *src, const uint32_t index0, const uint32_t count, const QueryRay &q, float &closest, uint32_t &hit, bool &active)
{
    uint32_t i = 0;
    for (; i + 4 <= count; i += 4) {
        OpenTest r[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t j = i + k;
            r[k] = test_triangle_open(unpack(src[4 * j + 0], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]), q.o, q.d);
        }
        asm volatile("" ::"v"(r[0].tt), "v"(r[0].m), "v"(r[0].s), "v"(r[1].tt), "v"(r[1].m), "v"(r[1].s), "v"(r[2].tt), "v"(r[2].m), "v"(r[2].s), "v"(r[3].tt),
                     "v"(r[3].m), "v"(r[3].s));
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) accept_query(r[k], index0 + i + k, q.any, closest, hit, active);
    }
    for (; i < count; ++i)
        accept_query(test_triangle_open(unpack(src[4 * i + 0], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]), q.o, q.d), index0 + i, q.any, closest, hit, active);
}

// the next run of 64 records for this wave (wave-uniform)
__device__ __forceinline__ uint32_t claim_run(uint32_t *counter, const uint32_t lane)
{
    uint32_t run = 0;
    if (lane == 0) run = atomicAdd(counter, 1u);
    return __builtin_amdgcn_readlane(run, 0);
}

}  // namespace

// rvpt_bvh4.hip's per-lane walk: slab_entry at the root, four slab_child tests per wide node, on with the first child that passes, the others stacked (the last
// first) with their entry distances and packed heads, popped with closest >= entry.  LDS: [stack: lds_levels x 2 words x kBlock][root: 2 float4][top_nodes wide nodes]
__global__ __launch_bounds__(kBlock) void query_bvh4(const QueryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t lds_levels = a.lds_levels;
    float4 *lds_root = reinterpret_cast<float4 *>(lds_stack + 2u * lds_levels * kBlock);
    float4 *lds_top = lds_root + 2;
    const uint32_t top_nodes = a.top_nodes;
    if (threadIdx.x < 2u) lds_root[threadIdx.x] = a.nodes[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < 8u * top_nodes; i += kBlock) lds_top[i] = a.wide[i];
    __syncthreads();
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t top_level = a.stack_levels - 1u;
    const uint32_t head_shift = a.head_shift;
    uint32_t *const ovf = a.stack_overflow + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x);
    const size_t ovf_stride = static_cast<size_t>(gridDim.x) * kBlock;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;
        const bool live = r < a.n;
        const QueryRay q = load_ray(a.records, r, live);
        float closest = __uint_as_float(q.tmax_bits);
        uint32_t hit = kNoPrim, sp = 0, cur = 0, leaf_first = 0, leaf_count = 0;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        {
            float entry;  // the root is a node like any other: its own box first (intersection.glsl:369-380)
            walking = walking && slab_entry(q.o, inv, lds_root[0], lds_root[1], closest, entry);
        }
        auto enter = [&](const uint32_t head) {  // head = first | count << head_shift (leaf, count > 0) or a wide node index (count 0)
            const uint32_t first = head & ((1u << head_shift) - 1u), count = head >> head_shift;
            cur = first;
            leaf_first = first;
            leaf_count = count;
        };
        auto push = [&](const float entry, const uint32_t head) {
            const uint32_t at = min(sp, top_level);  // the host sized the stack from the wide tree: sp never passes top_level; the clamp keeps a wrong size inside the memory
            if (at < lds_levels) {
                lds_stack[(2u * at + 0u) * kBlock + threadIdx.x] = __float_as_uint(entry);
                lds_stack[(2u * at + 1u) * kBlock + threadIdx.x] = head;
            } else {
                ovf[(2u * (at - lds_levels) + 0u) * ovf_stride] = __float_as_uint(entry);
                ovf[(2u * (at - lds_levels) + 1u) * ovf_stride] = head;
            }
            sp = at + 1u;
        };
        while (ballot(walking) != 0) {  // (any hit: a lane that accepted has left; the loop ends for the wave when none walks)
            bool need_pop = false;
            if (walking && leaf_count == 0) {
                const float4 *node = cur < top_nodes ? lds_top + 8u * cur : a.wide + 8u * static_cast<size_t>(cur);
                const float4 minx = node[0], maxx = node[1], miny = node[2], maxy = node[3], minz = node[4], maxz = node[5], hq = node[6];
                const uint32_t hd0 = __float_as_uint(hq.x), hd1 = __float_as_uint(hq.y), hd2 = __float_as_uint(hq.z), hd3 = __float_as_uint(hq.w);
                float e0, e1, e2, e3;
                const bool h0 = slab_child(q.o, inv, minx.x, maxx.x, miny.x, maxy.x, minz.x, maxz.x, closest, e0);  // (a wide node has at least two children)
                const bool h1 = slab_child(q.o, inv, minx.y, maxx.y, miny.y, maxy.y, minz.y, maxz.y, closest, e1);
                const bool h2 = slab_child(q.o, inv, minx.z, maxx.z, miny.z, maxy.z, minz.z, maxz.z, closest, e2) && hd2 != kWideEmpty;
                const bool h3 = slab_child(q.o, inv, minx.w, maxx.w, miny.w, maxy.w, minz.w, maxz.w, closest, e3) && hd3 != kWideEmpty;
                if (h3 && (h0 || h1 || h2)) push(e3, hd3);
                if (h2 && (h0 || h1)) push(e2, hd2);
                if (h1 && h0) push(e1, hd1);
                if (h0 || h1 || h2 || h3)
                    enter(h0 ? hd0 : (h1 ? hd1 : (h2 ? hd2 : hd3)));
                else
                    need_pop = true;
            }
            if (walking && leaf_count > 0) {
                if (test_leaf(prep, leaf_first, leaf_count, q, closest, hit)) walking = false;
                leaf_count = 0;
                need_pop = true;
            }
            if (walking && need_pop) {
                bool found = false;
                while (sp > 0 && !found) {
                    sp -= 1;
                    uint32_t entry_bits, cand;
                    if (sp < lds_levels) {
                        entry_bits = lds_stack[(2u * sp + 0u) * kBlock + threadIdx.x];
                        cand = lds_stack[(2u * sp + 1u) * kBlock + threadIdx.x];
                    } else {
                        entry_bits = ovf[(2u * (sp - lds_levels) + 0u) * ovf_stride];
                        cand = ovf[(2u * (sp - lds_levels) + 1u) * ovf_stride];
                    }
                    if (closest >= __uint_as_float(entry_bits)) {  // the reference's box test at the visit (rvpt_bvh4.hip's header comment)
                        enter(cand);
                        found = true;
                    }
                }
                walking = found;
            }
        }
        if (live) store_hit(a.records, r, q, a.prep, a.perm, closest, hit);
    }
}

// intersect_bvh as the reference writes it, over the binary nodes (children of an inner node at first, first + 1): pop a node, test its box against the interval
// of that moment, a leaf's triangles in order, an inner node's right child stacked and its left child next.  One word per stack slot (the node index); the LDS
// part uses the first word of query_bvh4's two-word slots, the global part the first half of its columns.
__global__ __launch_bounds__(kBlock) void query_bvh2(const QueryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t lds_levels = a.lds_levels;
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t top_level = a.stack_levels - 1u;
    uint32_t *const ovf = a.stack_overflow + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x);
    const size_t ovf_stride = static_cast<size_t>(gridDim.x) * kBlock;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;
        const bool live = r < a.n;
        const QueryRay q = load_ray(a.records, r, live);
        float closest = __uint_as_float(q.tmax_bits);
        uint32_t hit = kNoPrim, sp = 0, cur = 0;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        while (ballot(walking) != 0) {
            if (walking) {
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)], n1 = a.nodes[2u * static_cast<size_t>(cur) + 1u];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                float entry;
                if (slab_entry(q.o, inv, n0, n1, closest, entry)) {
                    if (count > 0) {
                        if (test_leaf(prep, first, count, q, closest, hit)) walking = false;
                    } else {
                        const uint32_t at = min(sp, top_level);  // (the tree's height bounds the pushes of a root-to-leaf path; the clamp as in query_bvh4)
                        if (at < lds_levels)
                            lds_stack[at * kBlock + threadIdx.x] = first + 1u;
                        else
                            ovf[(at - lds_levels) * ovf_stride] = first + 1u;
                        sp = at + 1u;
                        cur = first;
                        pop = false;
                    }
                }
                if (walking && pop) {
                    if (sp == 0) {
                        walking = false;
                    } else {
                        sp -= 1;
                        cur = sp < lds_levels ? lds_stack[sp * kBlock + threadIdx.x] : ovf[(sp - lds_levels) * ovf_stride];
                    }
                }
            }
        }
        if (live) store_hit(a.records, r, q, a.prep, a.perm, closest, hit);
    }
}

// Brute force: a work-group answers 256 records and streams the prepared triangles through LDS in tiles of kQueryTileTris; every lane runs over each tile in
// index order.  The loop ends for the work-group when no lane is left (every ray invalid, or every any-hit ray served).
__global__ __launch_bounds__(kBlock) void query_brute(const QueryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_tile[];
    const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = r < a.n;
    const QueryRay q = load_ray(a.records, r, live);
    float closest = __uint_as_float(q.tmax_bits);
    uint32_t hit = kNoPrim;
    bool active = q.valid;
    for (uint32_t base = 0; base < a.n_tris; base += kQueryTileTris) {
        const uint32_t count = min(kQueryTileTris, a.n_tris - base);
        for (uint32_t i = threadIdx.x; i < 4u * count; i += kBlock) lds_tile[i] = a.prep[4u * static_cast<size_t>(base) + i];
        __syncthreads();
        if (ballot(active) != 0) query_run(reinterpret_cast<const v4f *>(lds_tile), base, count, q, closest, hit, active);
        if (__syncthreads_or(active ? 1 : 0) == 0) break;  // (also the barrier in front of the next tile's stores)
    }
    if (live) store_hit(a.records, r, q, a.prep, a.perm, closest, hit);
}

// K-NEAREST RAY QUERIES (include/rvpt_hip.h: RVPT_HIP_FORMAT_RAY_HITS_NEAREST(k)): the three walks above with `closest` replaced by `bound`, the t of the k-th
// entry of a sorted list of hits a lane keeps in registers (the record's tmax until the list is full; an any-hit lane's bound stays tmax and its list is in
// the order of acceptance).  The walks never grow their interval, which is all the wide walk's equivalence with the binary one rests on.
namespace {

struct NearArgs {
    QueryArgs q;  // n, n_runs: GROUPS of k records, runs of 64 groups
    uint32_t k;   // hits per ray, 2 .. CAP (wave-uniform)
};

// CAP slots, t and the stored index of each, sorted by t (any hit: by acceptance); an empty slot is (+inf, kNoPrim) and empty slots come last.  An accepted
// t is below bound <= tmax, hence finite: no held hit compares above FLT_MAX, every empty slot does.  Slots at and past k fill like the others; nothing reads them.
// Constant indices only, every loop unrolled: the list stays in VGPRs.
template <int CAP>
struct HitList {
    float t[CAP];
    uint32_t index[CAP];
    float bound;  // the interval's end: tmax, or the k-th t once a closest-mode list holds k
    bool full;    // slot k - 1 is taken (an any-hit lane is finished)

    __device__ __forceinline__ void reset(const float tmax)
    {
#pragma unroll
        for (int j = 0; j < CAP; ++j) t[j] = kInf, index[j] = kNoPrim;
        bound = tmax;
        full = false;
    }
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
        bound = full && !any ? kth : tmax;
    }
};

// test_triangle's test against (0, bound), the chain entered only when some lane accepts
template <int CAP>
__device__ __forceinline__ void accept_near(const bool accept, const float tt, const uint32_t index, const QueryRay &q, const uint32_t k, HitList<CAP> &h)
{
    if (ballot(accept) != 0) {
        asm volatile("" ::: "memory");  // keep this a (wave-uniform) branch, as accept_hit does
        h.insert(accept, tt, index, q.any, __uint_as_float(q.tmax_bits), k);
    }
}

// test_leaf: a leaf's triangles in index order; true when an any-hit ray holds its k
template <int CAP>
__device__ __forceinline__ bool test_leaf_near(const v4f *prep, const uint32_t first, const uint32_t count, const QueryRay &q, const uint32_t k, HitList<CAP> &h)
{
    for (uint32_t i = first; i < first + count; ++i) {
        const v4f *tp = prep + 4 * static_cast<size_t>(i);
        const PrepTri t = unpack(tp[0], tp[1], tp[2], tp[3]);
        const float tt = div_dots(dot(t.v0 - q.o, t.n), dot(q.d, t.n));
        const f3 p0 = fma3(q.d, tt, q.o) - t.v0;
        const float b0 = dot(p0, t.e0);
        const float b1 = dot(p0, t.e1);
        const float u = t.inv_det * fma_(t.a01, b1, t.a00 * b0);
        const float v = t.inv_det * fma_(t.a11, b1, t.a01 * b0);
        accept_near((0.0f < tt) & (tt < h.bound) & (0.0f < u) & (0.0f < v) & (u + v < 1.0f), tt, i, q, k, h);
        if (q.any && h.full) return true;
    }
    return false;
}

// query_run for the brute-force kernel: four tests' arithmetic scheduled together, then the four accepts in order
template <int CAP>
__device__ __forceinline__ void near_run(const v4f *src, const uint32_t index0, const uint32_t count, const QueryRay &q, const uint32_t k, HitList<CAP> &h, bool &active)
{
    auto accept = [&](const OpenTest r, const uint32_t index) {
        accept_near((r.m > 0.0f) & (r.s < 1.0f) & (r.tt < h.bound) & active, r.tt, index, q, k, h);
        active = active && !(q.any && h.full);
    };
    uint32_t i = 0;
    for (; i + 4 <= count; i += 4) {
        OpenTest r[4];
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) {
            const uint32_t j = i + s;
            r[s] = test_triangle_open(unpack(src[4 * j + 0], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]), q.o, q.d);
        }
        asm volatile("" ::"v"(r[0].tt), "v"(r[0].m), "v"(r[0].s), "v"(r[1].tt), "v"(r[1].m), "v"(r[1].s), "v"(r[2].tt), "v"(r[2].m), "v"(r[2].s), "v"(r[3].tt),
                     "v"(r[3].m), "v"(r[3].s));
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) accept(r[s], index0 + i + s);
    }
    for (; i < count; ++i) accept(test_triangle_open(unpack(src[4 * i + 0], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]), q.o, q.d), index0 + i);
}

// A group's k out quads: slot j's hit with u and v recomputed as store_hit does (the same bits), the miss quad for an empty slot.  Only the third float4 of a
// record is stored, the followers' included.
template <int CAP>
__device__ __forceinline__ void store_hits(float4 *records, const size_t group, const QueryRay &q, const float4 *prep, const uint32_t *perm, const uint32_t k,
                                           const HitList<CAP> &h)
{
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (static_cast<uint32_t>(j) < k) store_hit(records, group * k + static_cast<uint32_t>(j), q, prep, perm, h.t[j], h.index[j]);
}

}  // namespace

// query_bvh4 with the list
template <int CAP>
__global__ __launch_bounds__(kBlock) void query_bvh4_near(const NearArgs na)
{
    const QueryArgs &a = na.q;
    const uint32_t k = na.k;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t lds_levels = a.lds_levels;
    float4 *lds_root = reinterpret_cast<float4 *>(lds_stack + 2u * lds_levels * kBlock);
    float4 *lds_top = lds_root + 2;
    const uint32_t top_nodes = a.top_nodes;
    if (threadIdx.x < 2u) lds_root[threadIdx.x] = a.nodes[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < 8u * top_nodes; i += kBlock) lds_top[i] = a.wide[i];
    __syncthreads();
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t top_level = a.stack_levels - 1u;
    const uint32_t head_shift = a.head_shift;
    uint32_t *const ovf = a.stack_overflow + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x);
    const size_t ovf_stride = static_cast<size_t>(gridDim.x) * kBlock;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t g = static_cast<size_t>(run) * 64u + lane;
        const bool live = g < a.n;
        const QueryRay q = load_ray(a.records, g * k, live);
        HitList<CAP> h;
        h.reset(__uint_as_float(q.tmax_bits));
        uint32_t sp = 0, cur = 0, leaf_first = 0, leaf_count = 0;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        {
            float entry;
            walking = walking && slab_entry(q.o, inv, lds_root[0], lds_root[1], h.bound, entry);
        }
        auto enter = [&](const uint32_t head) {
            const uint32_t first = head & ((1u << head_shift) - 1u), count = head >> head_shift;
            cur = first;
            leaf_first = first;
            leaf_count = count;
        };
        auto push = [&](const float entry, const uint32_t head) {
            const uint32_t at = min(sp, top_level);  // (the clamp keeps a wrong size inside the memory, as in query_bvh4)
            if (at < lds_levels) {
                lds_stack[(2u * at + 0u) * kBlock + threadIdx.x] = __float_as_uint(entry);
                lds_stack[(2u * at + 1u) * kBlock + threadIdx.x] = head;
            } else {
                ovf[(2u * (at - lds_levels) + 0u) * ovf_stride] = __float_as_uint(entry);
                ovf[(2u * (at - lds_levels) + 1u) * ovf_stride] = head;
            }
            sp = at + 1u;
        };
        while (ballot(walking) != 0) {
            bool need_pop = false;
            if (walking && leaf_count == 0) {
                const float4 *node = cur < top_nodes ? lds_top + 8u * cur : a.wide + 8u * static_cast<size_t>(cur);
                const float4 minx = node[0], maxx = node[1], miny = node[2], maxy = node[3], minz = node[4], maxz = node[5], hq = node[6];
                const uint32_t hd0 = __float_as_uint(hq.x), hd1 = __float_as_uint(hq.y), hd2 = __float_as_uint(hq.z), hd3 = __float_as_uint(hq.w);
                float e0, e1, e2, e3;
                const bool h0 = slab_child(q.o, inv, minx.x, maxx.x, miny.x, maxy.x, minz.x, maxz.x, h.bound, e0);
                const bool h1 = slab_child(q.o, inv, minx.y, maxx.y, miny.y, maxy.y, minz.y, maxz.y, h.bound, e1);
                const bool h2 = slab_child(q.o, inv, minx.z, maxx.z, miny.z, maxy.z, minz.z, maxz.z, h.bound, e2) && hd2 != kWideEmpty;
                const bool h3 = slab_child(q.o, inv, minx.w, maxx.w, miny.w, maxy.w, minz.w, maxz.w, h.bound, e3) && hd3 != kWideEmpty;
                if (h3 && (h0 || h1 || h2)) push(e3, hd3);
                if (h2 && (h0 || h1)) push(e2, hd2);
                if (h1 && h0) push(e1, hd1);
                if (h0 || h1 || h2 || h3)
                    enter(h0 ? hd0 : (h1 ? hd1 : (h2 ? hd2 : hd3)));
                else
                    need_pop = true;
            }
            if (walking && leaf_count > 0) {
                if (test_leaf_near(prep, leaf_first, leaf_count, q, k, h)) walking = false;
                leaf_count = 0;
                need_pop = true;
            }
            if (walking && need_pop) {
                bool found = false;
                while (sp > 0 && !found) {
                    sp -= 1;
                    uint32_t entry_bits, cand;
                    if (sp < lds_levels) {
                        entry_bits = lds_stack[(2u * sp + 0u) * kBlock + threadIdx.x];
                        cand = lds_stack[(2u * sp + 1u) * kBlock + threadIdx.x];
                    } else {
                        entry_bits = ovf[(2u * (sp - lds_levels) + 0u) * ovf_stride];
                        cand = ovf[(2u * (sp - lds_levels) + 1u) * ovf_stride];
                    }
                    if (h.bound >= __uint_as_float(entry_bits)) {  // the box test at the visit, against the interval of that moment
                        enter(cand);
                        found = true;
                    }
                }
                walking = found;
            }
        }
        if (live) store_hits(a.records, g, q, a.prep, a.perm, k, h);
    }
}

// query_bvh2 with the list
template <int CAP>
__global__ __launch_bounds__(kBlock) void query_bvh2_near(const NearArgs na)
{
    const QueryArgs &a = na.q;
    const uint32_t k = na.k;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t lds_levels = a.lds_levels;
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t top_level = a.stack_levels - 1u;
    uint32_t *const ovf = a.stack_overflow + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x);
    const size_t ovf_stride = static_cast<size_t>(gridDim.x) * kBlock;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t g = static_cast<size_t>(run) * 64u + lane;
        const bool live = g < a.n;
        const QueryRay q = load_ray(a.records, g * k, live);
        HitList<CAP> h;
        h.reset(__uint_as_float(q.tmax_bits));
        uint32_t sp = 0, cur = 0;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        while (ballot(walking) != 0) {
            if (walking) {
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)], n1 = a.nodes[2u * static_cast<size_t>(cur) + 1u];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                float entry;
                if (slab_entry(q.o, inv, n0, n1, h.bound, entry)) {
                    if (count > 0) {
                        if (test_leaf_near(prep, first, count, q, k, h)) walking = false;
                    } else {
                        const uint32_t at = min(sp, top_level);
                        if (at < lds_levels)
                            lds_stack[at * kBlock + threadIdx.x] = first + 1u;
                        else
                            ovf[(at - lds_levels) * ovf_stride] = first + 1u;
                        sp = at + 1u;
                        cur = first;
                        pop = false;
                    }
                }
                if (walking && pop) {
                    if (sp == 0) {
                        walking = false;
                    } else {
                        sp -= 1;
                        cur = sp < lds_levels ? lds_stack[sp * kBlock + threadIdx.x] : ovf[(sp - lds_levels) * ovf_stride];
                    }
                }
            }
        }
        if (live) store_hits(a.records, g, q, a.prep, a.perm, k, h);
    }
}

// query_brute with the list: a work-group answers 256 groups
template <int CAP>
__global__ __launch_bounds__(kBlock) void query_brute_near(const NearArgs na)
{
    const QueryArgs &a = na.q;
    const uint32_t k = na.k;
    extern __shared__ __attribute__((aligned(16))) float4 lds_tile[];
    const size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = g < a.n;
    const QueryRay q = load_ray(a.records, g * k, live);
    HitList<CAP> h;
    h.reset(__uint_as_float(q.tmax_bits));
    bool active = q.valid;
    for (uint32_t base = 0; base < a.n_tris; base += kQueryTileTris) {
        const uint32_t count = min(kQueryTileTris, a.n_tris - base);
        for (uint32_t i = threadIdx.x; i < 4u * count; i += kBlock) lds_tile[i] = a.prep[4u * static_cast<size_t>(base) + i];
        __syncthreads();
        if (ballot(active) != 0) near_run(reinterpret_cast<const v4f *>(lds_tile), base, count, q, k, h, active);
        if (__syncthreads_or(active ? 1 : 0) == 0) break;
    }
    if (live) store_hits(a.records, g, q, a.prep, a.perm, k, h);
}

namespace {

using NearKernel = void (*)(NearArgs);
// the smallest instance that holds k (2, 4 or 8 slots)
NearKernel near_kernel(const QueryKind kind, const uint32_t k)
{
    if (kind == QueryKind::Brute) return k <= 2u ? query_brute_near<2> : (k <= 4u ? query_brute_near<4> : query_brute_near<8>);
    if (kind == QueryKind::Wide) return k <= 2u ? query_bvh4_near<2> : (k <= 4u ? query_bvh4_near<4> : query_bvh4_near<8>);
    return k <= 2u ? query_bvh2_near<2> : (k <= 4u ? query_bvh2_near<4> : query_bvh2_near<8>);
}

}  // namespace

// RAY CROSSINGS (include/rvpt_hip.h: RVPT_HIP_FORMAT_RAY_CROSSINGS): the three walks once more, reduced instead of listed.  The interval is (0, tmax) from
// start to end, so the set of accepted tests is that of an any-hit k-nearest walk with no limit on k and does not depend on the visiting order; a lane keeps
// two counts and the smallest and largest accepted t, and never leaves its walk early.
namespace {

struct CrossArgs {
    QueryArgs q;
    const float4 *unit_n;  // n_tris: (normalize(n), 0) by stored index, as SURFACE POINTS returns it
};

struct Crossings {
    uint32_t front, back;
    float t_near, t_far;  // +inf and +0 while nothing is accepted: an accepted t is in (0, tmax), finite and positive
};

// An accepted test counts by its facing: s = (d.x n.x + d.y n.y) + d.z n.z, every operation rounded on its own; FRONT iff s < 0, everything else (s NaN
// included) BACK.  The normal is gathered only by the lanes that accept, and only when some lane does.
__device__ __forceinline__ void accept_cross(const bool accept, const float tt, const uint32_t index, const f3 d, const float4 *unit_n, Crossings &c)
{
    if (ballot(accept) != 0) {
        asm volatile("" ::: "memory");  // keep this a (wave-uniform) branch, as accept_hit does
        if (accept) {
            const float4 un = unit_n[index];
            const float s = __fadd_rn(__fadd_rn(__fmul_rn(d.x, un.x), __fmul_rn(d.y, un.y)), __fmul_rn(d.z, un.z));
            const bool front = s < 0.0f;
            c.front += front ? 1u : 0u;
            c.back += front ? 0u : 1u;
            c.t_near = __builtin_fminf(c.t_near, tt);
            c.t_far = __builtin_fmaxf(c.t_far, tt);
        }
    }
}

// test_leaf against the fixed interval: every triangle of the leaf, no early return
__device__ __forceinline__ void test_leaf_cross(const v4f *prep, const uint32_t first, const uint32_t count, const QueryRay &q, const float4 *unit_n, Crossings &c)
{
    const float tmax = __uint_as_float(q.tmax_bits);
    for (uint32_t i = first; i < first + count; ++i) {
        const v4f *tp = prep + 4 * static_cast<size_t>(i);
        const PrepTri t = unpack(tp[0], tp[1], tp[2], tp[3]);
        const float tt = div_dots(dot(t.v0 - q.o, t.n), dot(q.d, t.n));
        const f3 p0 = fma3(q.d, tt, q.o) - t.v0;
        const float b0 = dot(p0, t.e0);
        const float b1 = dot(p0, t.e1);
        const float u = t.inv_det * fma_(t.a01, b1, t.a00 * b0);
        const float v = t.inv_det * fma_(t.a11, b1, t.a01 * b0);
        accept_cross((0.0f < tt) & (tt < tmax) & (0.0f < u) & (0.0f < v) & (u + v < 1.0f), tt, i, q.d, unit_n, c);
    }
}

// query_run against the fixed interval (`active`: the ray is valid)
__device__ __forceinline__ void cross_run(const v4f *src, const uint32_t index0, const uint32_t count, const QueryRay &q, const float4 *unit_n, const bool active,
                                          Crossings &c)
{
    const float tmax = __uint_as_float(q.tmax_bits);
    auto accept = [&](const OpenTest r, const uint32_t index) {
        accept_cross((r.m > 0.0f) & (r.s < 1.0f) & (r.tt < tmax) & active, r.tt, index, q.d, unit_n, c);
    };
    uint32_t i = 0;
    for (; i + 4 <= count; i += 4) {
        OpenTest r[4];
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) {
            const uint32_t j = i + s;
            r[s] = test_triangle_open(unpack(src[4 * j + 0], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]), q.o, q.d);
        }
        asm volatile("" ::"v"(r[0].tt), "v"(r[0].m), "v"(r[0].s), "v"(r[1].tt), "v"(r[1].m), "v"(r[1].s), "v"(r[2].tt), "v"(r[2].m), "v"(r[2].s), "v"(r[3].tt),
                     "v"(r[3].m), "v"(r[3].s));
#pragma unroll
        for (uint32_t s = 0; s < 4; ++s) accept(r[s], index0 + i + s);
    }
    for (; i < count; ++i) accept(test_triangle_open(unpack(src[4 * i + 0], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]), q.o, q.d), index0 + i);
}

// A record's out quad: the counts, t_near and t_far; with nothing accepted (0, 0, the bits of tmax as given, +0)
__device__ __forceinline__ void store_crossings(float4 *records, const size_t r, const QueryRay &q, const Crossings &c)
{
    const bool none = (c.front | c.back) == 0u;
    records[3 * r + 2] = make_float4(__uint_as_float(c.front), __uint_as_float(c.back), none ? __uint_as_float(q.tmax_bits) : c.t_near, c.t_far);
}

}  // namespace

// query_bvh4 with the interval fixed at tmax: the stacked entry distances are still compared against it at the pop
__global__ __launch_bounds__(kBlock) void cross_bvh4(const CrossArgs ca)
{
    const QueryArgs &a = ca.q;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t lds_levels = a.lds_levels;
    float4 *lds_root = reinterpret_cast<float4 *>(lds_stack + 2u * lds_levels * kBlock);
    float4 *lds_top = lds_root + 2;
    const uint32_t top_nodes = a.top_nodes;
    if (threadIdx.x < 2u) lds_root[threadIdx.x] = a.nodes[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < 8u * top_nodes; i += kBlock) lds_top[i] = a.wide[i];
    __syncthreads();
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t top_level = a.stack_levels - 1u;
    const uint32_t head_shift = a.head_shift;
    uint32_t *const ovf = a.stack_overflow + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x);
    const size_t ovf_stride = static_cast<size_t>(gridDim.x) * kBlock;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;
        const bool live = r < a.n;
        const QueryRay q = load_ray(a.records, r, live);
        const float tmax = __uint_as_float(q.tmax_bits);
        Crossings c{0u, 0u, kInf, 0.0f};
        uint32_t sp = 0, cur = 0, leaf_first = 0, leaf_count = 0;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        {
            float entry;
            walking = walking && slab_entry(q.o, inv, lds_root[0], lds_root[1], tmax, entry);
        }
        auto enter = [&](const uint32_t head) {
            const uint32_t first = head & ((1u << head_shift) - 1u), count = head >> head_shift;
            cur = first;
            leaf_first = first;
            leaf_count = count;
        };
        auto push = [&](const float entry, const uint32_t head) {
            const uint32_t at = min(sp, top_level);  // (the clamp keeps a wrong size inside the memory, as in query_bvh4)
            if (at < lds_levels) {
                lds_stack[(2u * at + 0u) * kBlock + threadIdx.x] = __float_as_uint(entry);
                lds_stack[(2u * at + 1u) * kBlock + threadIdx.x] = head;
            } else {
                ovf[(2u * (at - lds_levels) + 0u) * ovf_stride] = __float_as_uint(entry);
                ovf[(2u * (at - lds_levels) + 1u) * ovf_stride] = head;
            }
            sp = at + 1u;
        };
        while (ballot(walking) != 0) {
            bool need_pop = false;
            if (walking && leaf_count == 0) {
                const float4 *node = cur < top_nodes ? lds_top + 8u * cur : a.wide + 8u * static_cast<size_t>(cur);
                const float4 minx = node[0], maxx = node[1], miny = node[2], maxy = node[3], minz = node[4], maxz = node[5], hq = node[6];
                const uint32_t hd0 = __float_as_uint(hq.x), hd1 = __float_as_uint(hq.y), hd2 = __float_as_uint(hq.z), hd3 = __float_as_uint(hq.w);
                float e0, e1, e2, e3;
                const bool h0 = slab_child(q.o, inv, minx.x, maxx.x, miny.x, maxy.x, minz.x, maxz.x, tmax, e0);
                const bool h1 = slab_child(q.o, inv, minx.y, maxx.y, miny.y, maxy.y, minz.y, maxz.y, tmax, e1);
                const bool h2 = slab_child(q.o, inv, minx.z, maxx.z, miny.z, maxy.z, minz.z, maxz.z, tmax, e2) && hd2 != kWideEmpty;
                const bool h3 = slab_child(q.o, inv, minx.w, maxx.w, miny.w, maxy.w, minz.w, maxz.w, tmax, e3) && hd3 != kWideEmpty;
                if (h3 && (h0 || h1 || h2)) push(e3, hd3);
                if (h2 && (h0 || h1)) push(e2, hd2);
                if (h1 && h0) push(e1, hd1);
                if (h0 || h1 || h2 || h3)
                    enter(h0 ? hd0 : (h1 ? hd1 : (h2 ? hd2 : hd3)));
                else
                    need_pop = true;
            }
            if (walking && leaf_count > 0) {
                test_leaf_cross(prep, leaf_first, leaf_count, q, ca.unit_n, c);
                leaf_count = 0;
                need_pop = true;
            }
            if (walking && need_pop) {
                bool found = false;
                while (sp > 0 && !found) {
                    sp -= 1;
                    uint32_t entry_bits, cand;
                    if (sp < lds_levels) {
                        entry_bits = lds_stack[(2u * sp + 0u) * kBlock + threadIdx.x];
                        cand = lds_stack[(2u * sp + 1u) * kBlock + threadIdx.x];
                    } else {
                        entry_bits = ovf[(2u * (sp - lds_levels) + 0u) * ovf_stride];
                        cand = ovf[(2u * (sp - lds_levels) + 1u) * ovf_stride];
                    }
                    if (tmax >= __uint_as_float(entry_bits)) {  // the box test at the visit: the interval is the one the child was stacked under
                        enter(cand);
                        found = true;
                    }
                }
                walking = found;
            }
        }
        if (live) store_crossings(a.records, r, q, c);
    }
}

// query_bvh2 with the interval fixed at tmax
__global__ __launch_bounds__(kBlock) void cross_bvh2(const CrossArgs ca)
{
    const QueryArgs &a = ca.q;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t lds_levels = a.lds_levels;
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const uint32_t top_level = a.stack_levels - 1u;
    uint32_t *const ovf = a.stack_overflow + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x);
    const size_t ovf_stride = static_cast<size_t>(gridDim.x) * kBlock;
    const uint32_t lane = lane_id();

    for (;;) {
        const uint32_t run = claim_run(a.counter, lane);
        if (run >= a.n_runs) break;
        const size_t r = static_cast<size_t>(run) * 64u + lane;
        const bool live = r < a.n;
        const QueryRay q = load_ray(a.records, r, live);
        const float tmax = __uint_as_float(q.tmax_bits);
        Crossings c{0u, 0u, kInf, 0.0f};
        uint32_t sp = 0, cur = 0;
        const f3 inv = mk(1.0f / q.d.x, 1.0f / q.d.y, 1.0f / q.d.z);
        bool walking = q.valid;
        while (ballot(walking) != 0) {
            if (walking) {
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)], n1 = a.nodes[2u * static_cast<size_t>(cur) + 1u];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                float entry;
                if (slab_entry(q.o, inv, n0, n1, tmax, entry)) {
                    if (count > 0) {
                        test_leaf_cross(prep, first, count, q, ca.unit_n, c);
                    } else {
                        const uint32_t at = min(sp, top_level);  // (the clamp as in query_bvh4)
                        if (at < lds_levels)
                            lds_stack[at * kBlock + threadIdx.x] = first + 1u;
                        else
                            ovf[(at - lds_levels) * ovf_stride] = first + 1u;
                        sp = at + 1u;
                        cur = first;
                        pop = false;
                    }
                }
                if (pop) {
                    if (sp == 0) {
                        walking = false;
                    } else {
                        sp -= 1;
                        cur = sp < lds_levels ? lds_stack[sp * kBlock + threadIdx.x] : ovf[(sp - lds_levels) * ovf_stride];
                    }
                }
            }
        }
        if (live) store_crossings(a.records, r, q, c);
    }
}

// query_brute with the interval fixed at tmax: a work-group runs over every tile unless none of its rays is valid
__global__ __launch_bounds__(kBlock) void cross_brute(const CrossArgs ca)
{
    const QueryArgs &a = ca.q;
    extern __shared__ __attribute__((aligned(16))) float4 lds_tile[];
    const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = r < a.n;
    const QueryRay q = load_ray(a.records, r, live);
    Crossings c{0u, 0u, kInf, 0.0f};
    const bool active = q.valid;
    if (__syncthreads_or(active ? 1 : 0) != 0) {
        for (uint32_t base = 0; base < a.n_tris; base += kQueryTileTris) {
            const uint32_t count = min(kQueryTileTris, a.n_tris - base);
            if (base != 0) __syncthreads();  // the last tile has been read by every wave
            for (uint32_t i = threadIdx.x; i < 4u * count; i += kBlock) lds_tile[i] = a.prep[4u * static_cast<size_t>(base) + i];
            __syncthreads();
            if (ballot(active) != 0) cross_run(reinterpret_cast<const v4f *>(lds_tile), base, count, q, ca.unit_n, active, c);
        }
    }
    if (live) store_crossings(a.records, r, q, c);
}

namespace {

// The persistent grid and the split of the stack for a tree walk by `kernel` (whose occupancy sizes the grid)
hipError_t plan_walk(const QueryScene &scene, const uint32_t n, const int num_cus, const void *kernel, QueryPlan *plan)
{
    QueryPlan p{};
    const uint32_t levels = std::max<uint32_t>(1u, scene.stack_levels);
    p.lds_levels = std::min(levels, kQueryLdsLevels);
    p.top_nodes = scene.kind == QueryKind::Wide ? std::min(scene.n_wide, kQueryTopNodes) : 0u;
    p.lds_bytes = static_cast<size_t>(p.lds_levels) * kBlock * 2u * sizeof(uint32_t) + 2u * sizeof(float4) + static_cast<size_t>(p.top_nodes) * 128u;
    int per_cu = 0;
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

QueryPlan plan_brute(const uint32_t n)
{
    QueryPlan p{};
    p.grid = std::max<uint32_t>(1u, static_cast<uint32_t>((static_cast<uint64_t>(n) + kBlock - 1u) / kBlock));
    p.lds_bytes = static_cast<size_t>(kQueryTileTris) * 64u;
    return p;
}

QueryArgs query_args(const QueryScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n)
{
    QueryArgs a{};
    a.prep = scene.prep, a.nodes = scene.nodes, a.wide = scene.wide, a.perm = scene.perm;
    a.records = static_cast<float4 *>(records);
    a.n = n;
    a.n_runs = static_cast<uint32_t>((static_cast<uint64_t>(n) + 63u) / 64u);
    a.counter = scratch;
    a.stack_overflow = scratch + 64;
    a.n_tris = scene.n_tris, a.head_shift = scene.head_shift;
    a.stack_levels = std::max<uint32_t>(1u, scene.stack_levels);
    a.lds_levels = plan.lds_levels, a.top_nodes = plan.top_nodes;
    return a;
}

}  // namespace

hipError_t cross_plan(const QueryScene &scene, const uint32_t n, const int num_cus, QueryPlan *plan)
{
    if (scene.kind == QueryKind::Brute) {
        *plan = plan_brute(n);
        return hipSuccess;
    }
    return plan_walk(scene, n, num_cus, scene.kind == QueryKind::Wide ? reinterpret_cast<const void *>(cross_bvh4) : reinterpret_cast<const void *>(cross_bvh2), plan);
}

hipError_t cross_launch(hipStream_t stream, const QueryScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n)
{
    if (n == 0) return hipSuccess;
    if (scene.n_tris > 0 && !scene.unit_n) return hipErrorInvalidValue;
    const CrossArgs ca{query_args(scene, plan, scratch, records, n), scene.unit_n};
    if (scene.kind == QueryKind::Brute) {
        hipLaunchKernelGGL(cross_brute, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, ca);
        return hipGetLastError();
    }
    const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (scene.kind == QueryKind::Wide)
        hipLaunchKernelGGL(cross_bvh4, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, ca);
    else
        hipLaunchKernelGGL(cross_bvh2, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, ca);
    return hipGetLastError();
}

hipError_t query_plan(const QueryScene &scene, const uint32_t n, const int num_cus, QueryPlan *plan, const uint32_t k)
{
    if (scene.kind == QueryKind::Brute) {
        *plan = plan_brute(n);
        return hipSuccess;
    }
    // (the occupancy of the instance that is launched: a k-nearest instance holds its list in registers and may fit fewer waves)
    const void *kernel = k > 1u ? reinterpret_cast<const void *>(near_kernel(scene.kind, k))
                                : (scene.kind == QueryKind::Wide ? reinterpret_cast<const void *>(query_bvh4) : reinterpret_cast<const void *>(query_bvh2));
    return plan_walk(scene, n, num_cus, kernel, plan);
}

hipError_t query_launch(hipStream_t stream, const QueryScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n, const uint32_t k)
{
    if (n == 0) return hipSuccess;
    if (k == 0 || k > kQueryMaxHits) return hipErrorInvalidValue;
    const QueryArgs a = query_args(scene, plan, scratch, records, n);
    if (k > 1u) {  // n groups of k records; k = 1 is format 2 itself, through the kernels below
        if (scene.kind != QueryKind::Brute) {
            const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
            if (e != hipSuccess) return e;
        }
        const NearArgs na{a, k};
        hipLaunchKernelGGL(near_kernel(scene.kind, k), dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, na);
        return hipGetLastError();
    }
    if (scene.kind == QueryKind::Brute) {
        hipLaunchKernelGGL(query_brute, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
        return hipGetLastError();
    }
    const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (scene.kind == QueryKind::Wide)
        hipLaunchKernelGGL(query_bvh4, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
    else
        hipLaunchKernelGGL(query_bvh2, dim3(plan.grid), dim3(kBlock), plan.lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace rv
