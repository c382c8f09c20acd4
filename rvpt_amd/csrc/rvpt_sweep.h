// rvpt_sweep.h — sphere sweeps (include/rvpt_hip.h: RVPT_HIP_FORMAT_SPHERE_SWEEPS): when and where a caller's moving spheres first touch the mesh, in place.  The
// kernels live in rvpt_sweep.hip; rvpt_abi.hip validates, stages host records and owns the buffers (the ray queries' staging buffer and scratch: rvpt_query.h).
// THE PER-TRIANGLE ARITHMETIC of the header — the slab test of the own box, the seven features, the reported time — is below, host and device: both kernels
// call sweep_candidate(), the walk calls sweep_slab() on its nodes, and rvpt_amd/host/host_sweep_table.cpp evaluates the same functions on the CPU for
// tests/test_sweep_host.py to hold against the numpy statement (rvpt_amd/scene.py: sweep_sphere_triangles), bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rvpt_math.h"
#include "rvpt_nearest.h"

namespace rv {

constexpr uint32_t kSweepRecordBytes = 48;  // sizeof(rvpt_sphere_sweep): three float4

// The launch shape for n records (QueryPlan's fields as for ray queries; top_nodes is 0): a persistent grid sized from the occupancy of the kernel that will run
// for the tree walk, one work-group per 256 records for the brute-force kernel.  The scene is a point query's (rvpt_nearest.h): the vertex rows and the binary
// nodes.  A stack slot is two words, (t_in bits, node), in LDS and in the global column alike.
hipError_t sweep_plan(const NearestScene &scene, uint32_t n, int num_cus, QueryPlan *plan);
// Answers records[0 .. n) in place on `stream`.  `scratch` as for query_launch: 64 words (the first is the claim counter, zeroed here), then plan.stack_words.
hipError_t sweep_launch(hipStream_t stream, const NearestScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, uint32_t n);

#if defined(__HIPCC__)

// A record's in quads and what every triangle and every node needs of them, made once: inv = 1/dir per axis (never read where dir is 0), rr = radius*radius,
// dd = dot(dir, dir).  valid: org and dir finite, radius a finite number >= 0, tmax a number >= 0 (+inf allowed; -0.0 is 0).
struct SweepProbe {
    f3 p, d, inv;
    float r, rr, dd, tmax;
    bool valid;
};

RV_HD bool sweep_finite(const float x) { return __builtin_fabsf(x) < __builtin_inff(); }  // false for NaN and +-inf

RV_HD SweepProbe sweep_probe(const f3 p, const float r, const f3 d, const float tmax)
{
    SweepProbe q;
    q.p = p, q.d = d, q.r = r, q.tmax = tmax;
    q.inv = mk(1.0f / (d.x == 0.0f ? 1.0f : d.x), 1.0f / (d.y == 0.0f ? 1.0f : d.y), 1.0f / (d.z == 0.0f ? 1.0f : d.z));
    q.rr = r * r;
    q.dd = dot_rounded(d, d);
    q.valid = sweep_finite(p.x) && sweep_finite(p.y) && sweep_finite(p.z) && sweep_finite(d.x) && sweep_finite(d.y) && sweep_finite(d.z) && sweep_finite(r) && r >= 0.0f &&
              tmax >= 0.0f;
    return q;
}

// One axis of the slab test: the side pair [lo - r, hi + r], one rounded operation each.  dir == 0: two comparisons and no arithmetic.  Otherwise near / far are
// (L - p)*inv and (H - p)*inv by the sign of dir, and they move t_in / t_out through SELECTS: a NaN — a node's NaN side, 0 * inf — moves nothing.
RV_HD void sweep_slab_axis(const float p, const float d, const float inv, const float r, const float lo, const float hi, float &t_in, float &t_out, bool &outside)
{
    const float low = lo - r, high = hi + r;
    const bool zero = d == 0.0f;
    const float t1 = (low - p) * inv, t2 = (high - p) * inv;
    const float near = zero ? -__builtin_inff() : (d > 0.0f ? t1 : t2), far = zero ? __builtin_inff() : (d > 0.0f ? t2 : t1);
    outside = outside || (zero && (p < low || p > high));
    t_in = near > t_in ? near : t_in;
    t_out = far < t_out ? far : t_out;
}

// STEP 1 of the header, for a triangle's own box and for a node's alike: the centre's path over [0, tmax] against [lo - r, hi + r].  Passes iff no zero axis
// rejected, t_in <= t_out and t_in < +inf.  Every operation is monotone in lo and hi, so a box that contains another passes whenever that one does, with a t_in
// that is not larger: THE PRUNING LEMMA.
RV_HD bool sweep_slab(const SweepProbe &q, const f3 lo, const f3 hi, float &t_in)
{
    float t_out = q.tmax;
    bool outside = false;
    t_in = 0.0f;
    sweep_slab_axis(q.p.x, q.d.x, q.inv.x, q.r, lo.x, hi.x, t_in, t_out, outside);
    sweep_slab_axis(q.p.y, q.d.y, q.inv.y, q.r, lo.y, hi.y, t_in, t_out, outside);
    sweep_slab_axis(q.p.z, q.d.z, q.inv.z, q.r, lo.z, hi.z, t_in, t_out, outside);
    return !outside && t_in <= t_out && t_in < __builtin_inff();
}

// The smaller root of a0*t*t + 2*b0*t + c0 = 0 for a centre that starts outside (c0 > 0) and approaches (b0 < 0), as c0 / (sqrt(b0*b0 - a0*c0) - b0): no
// cancellation.  True iff the root exists and lies in [0, tmax].
RV_HD bool sweep_root(const float c0, const float b0, const float a0, const float tmax, float &t)
{
    const float disc = b0 * b0 - a0 * c0;
    const bool ok = c0 > 0.0f && b0 < 0.0f && a0 > 0.0f && disc >= 0.0f;
    t = c0 / (ok ? __builtin_sqrtf(disc) - b0 : 1.0f);
    return ok && t >= 0.0f && t <= tmax;
}

// One (vertex, edge) pair of STEP 2: the sphere about x0 and the infinite cylinder about the line x0 + s*e, e = x1 - x0, accepted where the contact projects
// into the edge.  m = p - x0 serves both.  Lowers t_tri to each time it accepts.
RV_HD void sweep_vertex_edge(const SweepProbe &q, const f3 x0, const f3 x1, float &t_tri)
{
    const f3 m = q.p - x0, e = x1 - x0;
    const float b = dot_rounded(m, q.d), c = dot_rounded(m, m) - q.rr;
    float t;
    const bool vertex_root = sweep_root(c, b, q.dd, q.tmax, t);
    const float t_vertex = c <= 0.0f ? 0.0f : (vertex_root ? t : __builtin_inff());
    t_tri = t_vertex < t_tri ? t_vertex : t_tri;
    const float ee = dot_rounded(e, e), md = dot_rounded(m, e), nd = dot_rounded(q.d, e);
    const float ca = ee * q.dd - nd * nd, cb = ee * b - nd * md, cc = ee * c - md * md;
    bool edge_root = sweep_root(cc, cb, ca, q.tmax, t) && ee > 0.0f;
    const float s = md + t * nd;
    edge_root = edge_root && s >= 0.0f && s <= ee;
    const bool inside = ee > 0.0f && cc <= 0.0f && md >= 0.0f && md <= ee;
    const float t_edge = inside ? 0.0f : (edge_root ? t : __builtin_inff());
    t_tri = t_edge < t_tri ? t_edge : t_tri;
}

// The face of STEP 2: the plane pushed out by r*|n| towards the centre's side, accepted iff closest_point() puts the centre at that time in region 0
RV_HD void sweep_face(const SweepProbe &q, const f3 a, const f3 b, const f3 c, float &t_tri)
{
    const f3 x = b - a, y = c - a;
    const f3 n = mk(x.y * y.z - x.z * y.y, x.z * y.x - x.x * y.z, x.x * y.y - x.y * y.x);
    const float nn = dot_rounded(n, n);
    const float h = dot_rounded(q.p - a, n);
    const float rn = q.r * __builtin_sqrtf(nn);
    const float hs = __builtin_fabsf(h), dn = dot_rounded(q.d, n);
    const float dns = h > 0.0f ? dn : -dn;
    const bool within = hs <= rn;
    const bool moving = !within && hs > rn && dns < 0.0f;
    float t = within ? 0.0f : (rn - hs) / (moving ? dns : 1.0f);
    const bool ok = nn > 0.0f && (within || (moving && t >= 0.0f && t <= q.tmax));
    t = ok ? t : 0.0f;
    const bool face = ok && closest_point(a, b, c, q.p + q.d * t).region == 0u;
    const float t_face = face ? t : __builtin_inff();
    t_tri = t_face < t_tri ? t_face : t_tri;
}

// STEP 2: the smallest contact time over the seven features, +inf where there is none
RV_HD float sweep_contact(const SweepProbe &q, const f3 a, const f3 b, const f3 c)
{
    float t_tri = __builtin_inff();
    sweep_vertex_edge(q, a, b, t_tri);
    sweep_vertex_edge(q, b, c, t_tri);
    sweep_vertex_edge(q, c, a, t_tri);
    sweep_face(q, a, b, c, t_tri);
    return t_tri;
}

RV_HD bool sweep_own_box(const SweepProbe &q, const f3 a, const f3 b, const f3 c, float &t_in)
{
    const bool finite = sweep_finite(a.x) && sweep_finite(a.y) && sweep_finite(a.z) && sweep_finite(b.x) && sweep_finite(b.y) && sweep_finite(b.z) && sweep_finite(c.x) &&
                        sweep_finite(c.y) && sweep_finite(c.z);
    const f3 lo = mk(__builtin_fminf(__builtin_fminf(a.x, b.x), c.x), __builtin_fminf(__builtin_fminf(a.y, b.y), c.y), __builtin_fminf(__builtin_fminf(a.z, b.z), c.z));
    const f3 hi = mk(__builtin_fmaxf(__builtin_fmaxf(a.x, b.x), c.x), __builtin_fmaxf(__builtin_fmaxf(a.y, b.y), c.y), __builtin_fmaxf(__builtin_fmaxf(a.z, b.z), c.z));
    return sweep_slab(q, lo, hi, t_in) && finite;
}

// STEP 3: the reported time behind a passed own box, t = t_in > t_tri ? t_in : t_tri; a candidate iff it is below +inf
RV_HD bool sweep_reported(const float t_in, const float t_tri, float &t)
{
    t = t_in > t_tri ? t_in : t_tri;
    return t < __builtin_inff();
}

// The candidate of one triangle, all steps (the host table's form; the kernels put a wave-uniform branch between the own box and the features)
RV_HD bool sweep_candidate(const SweepProbe &q, const f3 a, const f3 b, const f3 c, float &t)
{
    float t_in;
    t = 0.0f;
    if (!sweep_own_box(q, a, b, c, t_in)) return false;
    return sweep_reported(t_in, sweep_contact(q, a, b, c), t);
}

#endif  // __HIPCC__

}  // namespace rv
