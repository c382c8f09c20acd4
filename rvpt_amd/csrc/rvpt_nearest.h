// rvpt_nearest.h — point queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_NEAREST_POINTS): the nearest point of the mesh to a caller's points, in place.  The kernels
// live in rvpt_nearest.hip; rvpt_abi.hip validates, stages host records and owns the buffers (the ray queries' staging buffer and scratch: rvpt_query.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rvpt_math.h"
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

#if defined(__HIPCC__)

// THE PER-TRIANGLE ARITHMETIC of a point query (include/rvpt_hip.h: NEAREST POINTS), for the kernels of rvpt_nearest.hip and, through rvpt_sweep.h, for the
// sphere sweeps; host and device, so that a host program can hold it against the numpy statement.
struct Closest {
    f3 q;
    float d2, u, v;
    uint32_t region;
};

// (x0*y0 + x1*y1) + x2*y2, three products and two sums, each rounded (rv::dot of rvpt_math.h is the FUSED one: not used here)
RV_HD float dot_rounded(const f3 a, const f3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// the IEEE quotient; a quotient whose divisor is 0 is taken as 0
RV_HD float quotient(const float num, const float den) { return den == 0.0f ? 0.0f : num / den; }
RV_HD float clamp_keep_nan(const float q, const float lo, const float hi) { return q < lo ? lo : (q > hi ? hi : q); }

// The candidate of one triangle (a, b, c) for the point p: Ericson's point-triangle test, its regions tested in the specified order — written as selects over
// the seven predicates, which picks the first that holds exactly as the chain of ifs does — then q = (a + ab*u) + ac*v clamped into the triangle's own box.
// Two quotients at most (the face's u and v); every other region has one or none, and their operands are selected before the divide.
RV_HD Closest closest_point(const f3 a, const f3 b, const f3 c, const f3 p)
{
    const f3 ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c;
    const float d1 = dot_rounded(ab, ap), d2 = dot_rounded(ac, ap), d3 = dot_rounded(ab, bp), d4 = dot_rounded(ac, bp), d5 = dot_rounded(ab, cp), d6 = dot_rounded(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e1 = d4 - d3, e2 = d5 - d6;
    const bool r1 = d1 <= 0.0f && d2 <= 0.0f;
    const bool r2 = d3 >= 0.0f && d4 <= d3;
    const bool r4 = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool r3 = d6 >= 0.0f && d5 <= d6;
    const bool r5 = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool r6 = va <= 0.0f && e1 >= 0.0f && e2 >= 0.0f;
    const uint32_t region = r1 ? 1u : (r2 ? 2u : (r4 ? 4u : (r3 ? 3u : (r5 ? 5u : (r6 ? 6u : 0u)))));
    const float s = (va + vb) + vc;
    const float num_a = region == 4u ? d1 : (region == 5u ? d2 : (region == 6u ? e1 : vb));
    const float den_a = region == 4u ? d1 - d3 : (region == 5u ? d2 - d6 : (region == 6u ? e1 + e2 : s));
    const bool one = region >= 4u || region == 0u;  // the regions with a quotient
    const float qa = quotient(one ? num_a : 0.0f, one ? den_a : 1.0f);
    const float qb = quotient(region == 0u ? vc : 0.0f, region == 0u ? s : 1.0f);
    Closest r;
    r.region = region;
    r.u = region == 2u ? 1.0f : (region == 4u ? qa : (region == 6u ? 1.0f - qa : (region == 0u ? qa : 0.0f)));
    r.v = region == 3u ? 1.0f : (region == 5u ? qa : (region == 6u ? qa : (region == 0u ? qb : 0.0f)));
    const f3 raw = (a + ab * r.u) + ac * r.v;
    const f3 lo = mk(__builtin_fminf(__builtin_fminf(a.x, b.x), c.x), __builtin_fminf(__builtin_fminf(a.y, b.y), c.y), __builtin_fminf(__builtin_fminf(a.z, b.z), c.z));
    const f3 hi = mk(__builtin_fmaxf(__builtin_fmaxf(a.x, b.x), c.x), __builtin_fmaxf(__builtin_fmaxf(a.y, b.y), c.y), __builtin_fmaxf(__builtin_fmaxf(a.z, b.z), c.z));
    r.q = mk(clamp_keep_nan(raw.x, lo.x, hi.x), clamp_keep_nan(raw.y, lo.y, hi.y), clamp_keep_nan(raw.z, lo.z, hi.z));
    const f3 d = p - r.q;
    r.d2 = (d.x * d.x + d.y * d.y) + d.z * d.z;
    return r;
}

#endif  // __HIPCC__

}  // namespace rv
