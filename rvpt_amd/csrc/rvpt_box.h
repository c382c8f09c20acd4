// rvpt_box.h — box queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_BOX_OVERLAPS): how many triangles of the mesh meet a caller's boxes, and which, in place.  The
// kernels live in rvpt_box.hip; rvpt_abi.hip validates, stages host records and owns the buffers (the ray queries' staging buffer and scratch: rvpt_query.h).
// THE TEST of the header, triangle_meets_box() below, is the one function both kernels call.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rvpt_math.h"
#include "rvpt_nearest.h"

namespace rv {

constexpr uint32_t kBoxRecordBytes = 48;  // sizeof(rvpt_box_overlap): three float4
constexpr uint32_t kBoxMaxGroup = 4;      // RVPT_HIP_BOX_MAX_GROUP: the k of RVPT_HIP_FORMAT_BOX_OVERLAPS_K(k); a group lists 4k - 1 numbers in register lists of 3, 7 or 15 slots

// The launch shape for n GROUPS of k records, one box each (QueryPlan's fields as for ray queries; top_nodes is 0): a persistent grid sized from the occupancy
// of the instance that will run for the tree walk, one work-group per 256 groups for the brute-force kernel.  The scene is a point query's (rvpt_nearest.h):
// the vertex rows and the binary nodes.  A stack slot is ONE word here (a node index), in LDS and in the global column alike.
hipError_t box_plan(const NearestScene &scene, uint32_t n, int num_cus, QueryPlan *plan, uint32_t k);
// Answers the n groups records[0 .. n * k) in place on `stream`, the plan made with the same k.  `scratch` as for query_launch: 64 words (the first is the
// claim counter, zeroed here), then plan.stack_words.
hipError_t box_launch(hipStream_t stream, const NearestScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, uint32_t n, uint32_t k);

#if defined(__HIPCC__)

// A record's box as THE TEST uses it: lo, hi as given, ctr = lo*0.5 + hi*0.5 and h = hi - ctr (step 2; the same four operations per axis for every triangle,
// hence made once per box)
struct BoxProbe {
    f3 lo, hi, ctr, h;
};

__device__ __forceinline__ BoxProbe box_probe(const f3 lo, const f3 hi)
{
    BoxProbe q;
    q.lo = lo, q.hi = hi;
    q.ctr = mk(lo.x * 0.5f + hi.x * 0.5f, lo.y * 0.5f + hi.y * 0.5f, lo.z * 0.5f + hi.z * 0.5f);
    q.h = hi - q.ctr;
    return q;
}

// The six comparisons of step 1 against a box [blo, bhi] that contains what lies under it — a node's, or the triangle's own: true iff some comparison rejects.
// A NaN side rejects nothing.
__device__ __forceinline__ bool box_apart(const BoxProbe &q, const f3 blo, const f3 bhi)
{
    return blo.x > q.hi.x || bhi.x < q.lo.x || blo.y > q.hi.y || bhi.y < q.lo.y || blo.z > q.hi.z || bhi.z < q.lo.z;
}

// One edge axis of step 4: p_m = e1*v_m2 - e2*v_m1 over the two axes (k1, k2) of the cross product, r = h1*|e2| + h2*|e1|; "min(p) > r" is all three above r,
// "max(p) < -r" all three below -r, so that a NaN among them rejects nothing.
__device__ __forceinline__ bool edge_axis_apart(const float e1, const float e2, const float h1, const float h2, const float v01, const float v02, const float v11,
                                                const float v12, const float v21, const float v22)
{
    const float p0 = e1 * v02 - e2 * v01, p1 = e1 * v12 - e2 * v11, p2 = e1 * v22 - e2 * v21;
    const float r = h1 * __builtin_fabsf(e2) + h2 * __builtin_fabsf(e1);
    return (p0 > r && p1 > r && p2 > r) || (p0 < -r && p1 < -r && p2 < -r);
}

__device__ __forceinline__ bool edge_apart(const f3 e, const f3 h, const f3 v0, const f3 v1, const f3 v2)
{
    return edge_axis_apart(e.y, e.z, h.y, h.z, v0.y, v0.z, v1.y, v1.z, v2.y, v2.z) ||  // j = x: k1 = y, k2 = z
           edge_axis_apart(e.z, e.x, h.z, h.x, v0.z, v0.x, v1.z, v1.x, v2.z, v2.x) ||  // j = y: k1 = z, k2 = x
           edge_axis_apart(e.x, e.y, h.x, h.y, v0.x, v0.y, v1.x, v1.y, v2.x, v2.y);    // j = z: k1 = x, k2 = y
}

// THE TEST (include/rvpt_hip.h: BOX OVERLAPS; rvpt_amd/scene.py: triangle_box_overlaps states it in numpy): the rounded separating-axis test of the triangle
// (a, b, c) against the closed box, 13 axes, binary32 with every product, sum and difference rounded on its own (this translation unit is compiled with
// -ffp-contract=off like every other, and nothing here calls fma_()).  Every comparison is a rejection; a triangle with a non-finite component is never in.
__device__ __forceinline__ bool triangle_meets_box(const f3 a, const f3 b, const f3 c, const BoxProbe &q)
{
    const float big = __builtin_inff();
    const bool finite = __builtin_fabsf(a.x) < big && __builtin_fabsf(a.y) < big && __builtin_fabsf(a.z) < big && __builtin_fabsf(b.x) < big &&
                        __builtin_fabsf(b.y) < big && __builtin_fabsf(b.z) < big && __builtin_fabsf(c.x) < big && __builtin_fabsf(c.y) < big && __builtin_fabsf(c.z) < big;
    // 1. boxes: comparisons only
    const bool apart = (a.x > q.hi.x && b.x > q.hi.x && c.x > q.hi.x) || (a.x < q.lo.x && b.x < q.lo.x && c.x < q.lo.x) ||
                       (a.y > q.hi.y && b.y > q.hi.y && c.y > q.hi.y) || (a.y < q.lo.y && b.y < q.lo.y && c.y < q.lo.y) ||
                       (a.z > q.hi.z && b.z > q.hi.z && c.z > q.hi.z) || (a.z < q.lo.z && b.z < q.lo.z && c.z < q.lo.z);
    if (!finite || apart) return false;
    // 2. set-up
    const f3 h = q.h;
    const f3 v0 = a - q.ctr, v1 = b - q.ctr, v2 = c - q.ctr;
    const f3 e0 = b - a, e1 = c - b, e2 = a - c;
    // 3. the triangle's plane against the box's two extreme corners along n
    const f3 x = e0, y = c - a;
    const f3 n = mk(x.y * y.z - x.z * y.y, x.z * y.x - x.x * y.z, x.x * y.y - x.y * y.x);
    const f3 near = mk(n.x > 0.0f ? -h.x - v0.x : h.x - v0.x, n.y > 0.0f ? -h.y - v0.y : h.y - v0.y, n.z > 0.0f ? -h.z - v0.z : h.z - v0.z);
    const f3 far = mk(n.x > 0.0f ? h.x - v0.x : -h.x - v0.x, n.y > 0.0f ? h.y - v0.y : -h.y - v0.y, n.z > 0.0f ? h.z - v0.z : -h.z - v0.z);
    if ((n.x * near.x + n.y * near.y) + n.z * near.z > 0.0f) return false;
    if ((n.x * far.x + n.y * far.y) + n.z * far.z < 0.0f) return false;
    // 4. the nine edge axes
    return !(edge_apart(e0, h, v0, v1, v2) || edge_apart(e1, h, v0, v1, v2) || edge_apart(e2, h, v0, v1, v2));
}

#endif  // __HIPCC__

}  // namespace rv
