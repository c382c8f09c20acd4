// rvpt_vis.h — the bounce cull's table (the packet kernel's bounce rounds, rvpt_packets.hip): one word of one row.  Host + device, double
// precision on the float records taken as exact, no GPU needed (rvpt_bounce_rows, tests/test_bounce_rows.py).
//
// Row 2 A + s, bit B = 0 only when triangle B lies WHOLLY behind the plane of triangle A as seen from side s (s = 0: the side A's normal n = cross(e0, e1)
// points to) by more than `margin`, and both triangles are well shaped (sin^2 of the angle between the edges >= 2^-6, finite, non-degenerate).  A segment that
// leaves A on side s — origin on A's plane up to the float error of a position, pushed EPSILON towards s, direction with a non-negative component towards s
// (rvpt_device.h: shade, which says so in `leave` and gives up the cull where it cannot prove it) — cannot be accepted by the float test against such a B: the
// accepted point lies within (33 eps / kappa_B)(t + S) of B (rvpt_rect.h has the bound), far less than the margin of 2^-10 scene scales upload_scene passes.
#pragma once

#include <stdint.h>

#include "rvpt_math.h"

namespace rv {

// prep: n x 16 floats, the prepared records q0 = (v0, n.x) q1 = (n.yz, e0.xy) q2 = (e0.z, e1) q3 = Gram terms (rvpt_device.h)
RV_HD uint32_t bounce_row_word(const float *prep, const uint32_t n, const uint32_t row, const uint32_t w, const double margin)
{
    const uint32_t A = row >> 1;
    const double side = (row & 1u) ? -1.0 : 1.0;
    auto edges_ok = [](const double *e0, const double *e1) {  // sin^2 of the angle between the edges >= 2^-6 (NaN / degenerate: false)
        const double a00 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], a11 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2];
        const double a01 = e0[0] * e1[0] + e0[1] * e1[1] + e0[2] * e1[2];
        return (a00 * a11 - a01 * a01) >= 0x1p-6 * (a00 * a11) && a00 * a11 > 0.0;
    };
    const float *a = prep + 16u * A;
    const double av0[3] = {a[0], a[1], a[2]}, an[3] = {a[3], a[4], a[5]}, ae0[3] = {a[6], a[7], a[8]}, ae1[3] = {a[9], a[10], a[11]};
    const double nn = __builtin_sqrt(an[0] * an[0] + an[1] * an[1] + an[2] * an[2]);
    const bool a_ok = edges_ok(ae0, ae1) && nn > 0.0 && margin > 0.0;
    uint32_t bits = 0u;
    for (uint32_t b = 0; b < 32u; ++b) {
        const uint32_t B = 32u * w + b;
        if (B >= n) break;
        const float *q = prep + 16u * B;
        const double v0[3] = {q[0], q[1], q[2]}, e0[3] = {q[6], q[7], q[8]}, e1[3] = {q[9], q[10], q[11]};
        bool behind = a_ok && edges_ok(e0, e1);
        for (int k = 0; k < 3 && behind; ++k) {  // the three vertices of the record's triangle: v0, v0 + e0, v0 + e1
            const double p[3] = {v0[0] + (k == 1 ? e0[0] : (k == 2 ? e1[0] : 0.0)) - av0[0], v0[1] + (k == 1 ? e0[1] : (k == 2 ? e1[1] : 0.0)) - av0[1],
                                 v0[2] + (k == 1 ? e0[2] : (k == 2 ? e1[2] : 0.0)) - av0[2]};
            const double dist = side * (p[0] * an[0] + p[1] * an[1] + p[2] * an[2]) / nn;
            behind = dist <= -margin;  // (NaN: false -> the triangle stays in the row)
        }
        if (!behind) bits |= 1u << b;
    }
    return bits;
}

// what float errors of positions scale with: the largest |coordinate| + the largest extent of the uploaded triangles (reference Triangle records: 16 floats,
// vertices at [0..2], [4..6], [8..10]); 0 when a coordinate is not finite or the scale is absurd (then there is no table)
inline double bounce_scene_scale(const float *tris, const size_t n_tris)
{
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, amax = 0.0;
    bool finite = true;
    for (size_t i = 0; i < n_tris; ++i)
        for (int v = 0; v < 3; ++v)
            for (int k = 0; k < 3; ++k) {
                const double x = tris[16 * i + 4 * v + k];
                finite = finite && (x - x == 0.0);
                lo[k] = x < lo[k] ? x : lo[k], hi[k] = x > hi[k] ? x : hi[k];
                amax = (x < 0.0 ? -x : x) > amax ? (x < 0.0 ? -x : x) : amax;
            }
    double ext = hi[0] - lo[0];
    ext = (hi[1] - lo[1]) > ext ? (hi[1] - lo[1]) : ext;
    ext = (hi[2] - lo[2]) > ext ? (hi[2] - lo[2]) : ext;
    const double scale = amax + ext;
    return (n_tris > 0 && finite && scale > 0x1p-60 && scale < 0x1p60) ? scale : 0.0;
}
// ---- the leaf boxes of the bounce rounds (round 6) -------------------------------------------------------------------------------------------------------
// Triangles kLeafTris k .. kLeafTris k + kLeafTris - 1 of the uploaded buffer (the caller's order: BVH-leaf order at the reference's seam, rvpt.cpp:83-86 — spatially
// coherent; any other order only makes the boxes loose) share one axis-aligned box: the bounds of their records' triangles (v0, v0 + e0, v0 + e1 and the uploaded
// vertices themselves), widened by M = 2^-9 (scene scale + 2 EPSILON) on every side.  In a bounce round the wave keeps a group of kLeafTris candidate triangles only
// if SOME lane's ray passes the conservative slab test of the group's box (rvpt_device.h: leaf_slab).  A superset test — why an accepted pair always passes:
// the float test accepts only when the exact ray comes within E <= (33 eps / kappa)(t + S) of the record's triangle (rvpt_rect.h); for kappa >= 2^-6 — a leaf with a
// triangle below that, degenerate or non-finite gets the infinite box — E <= 2^-13 (t + S) <= 2^-10.4 (scale + EPSILON) (t <= twice the scene, S = four 1-norms of
// points of the scene or EPSILON off it), i.e. a point Y of the exact ray with t_Y > 0 lies inside the box widened by 0.4 M; the slab test evaluates
// fma(b, inv, -fl(o inv)) with inv = v_rcp_f32(d) (1 ulp; |inv| clamped to 2^60: an axis the ray does not move along by more than 2^-51 of the scene), whose error is
// <= 2^-21 (|b| + |o|) |inv| — 2^-12 of the remaining slack 0.6 M |inv|; so every axis' computed interval contains t_Y and the test passes.  Lanes whose segment is not
// covered by a proof (leave == all ones: the aa loop's camera rays, a Lambert direction that all but cancelled, eta > 16) vote for every box.
#ifndef RV_LEAF_TRIS
#define RV_LEAF_TRIS 8
#endif
constexpr uint32_t kLeafTris = RV_LEAF_TRIS;  // 4 or 8: a nibble or a byte of a row word
static_assert(kLeafTris == 4 || kLeafTris == 8, "a leaf is a nibble or a byte of a 32-triangle row word");
constexpr double kLeafBoxMarginScales = 0x1p-9;

// out: 8 floats per group of `group` consecutive triangles (lo.xyz, hi.xyz, 0, 0); tris: reference Triangle records (16 floats each), n_tris <= kResidentMaxTris;
// scale = bounce_scene_scale(tris).  group = kLeafTris: the leaf boxes; group = 1: every triangle's own box, tested (second level) for the triangles of a leaf that
// some ray came near, before the triangle itself — 16 VALU instead of 38 for the three in four that no ray of the round comes near
inline void bounce_group_boxes(const float *tris, const size_t n_tris, const double scale, const size_t group, float *out)
{
    const size_t kLeafTris = group;  // (shadows the constant: the body below is written for "a leaf")
    const size_t n_leaves = (n_tris + kLeafTris - 1) / kLeafTris;
    const double M = kLeafBoxMarginScales * (scale + 2.0 * 0.005);
    const float inf = __builtin_inff();
    for (size_t l = 0; l < n_leaves; ++l) {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        bool ok = true;
        for (size_t i = l * kLeafTris; i < n_tris && i < (l + 1) * kLeafTris; ++i) {
            const float *t = tris + 16 * i;
            const float v0[3] = {t[0], t[1], t[2]};
            float e0[3], e1[3];
            for (int k = 0; k < 3; ++k) e0[k] = t[4 + k] - v0[k], e1[k] = t[8 + k] - v0[k];  // prepare_triangles' float edges (rvpt_kernels.hip)
            const double a00 = double(e1[0]) * e1[0] + double(e1[1]) * e1[1] + double(e1[2]) * e1[2], a11 = double(e0[0]) * e0[0] + double(e0[1]) * e0[1] + double(e0[2]) * e0[2];
            const double a01 = double(e0[0]) * e1[0] + double(e0[1]) * e1[1] + double(e0[2]) * e1[2];
            ok = ok && (a00 * a11 - a01 * a01) >= 0x1p-6 * (a00 * a11) && a00 * a11 > 0.0;  // (NaN: false)
            for (int k = 0; k < 3; ++k) {
                const double c[5] = {v0[k], t[4 + k], t[8 + k], double(v0[k]) + e0[k], double(v0[k]) + e1[k]};
                for (double x : c) {
                    ok = ok && (x - x == 0.0);
                    lo[k] = x < lo[k] ? x : lo[k], hi[k] = x > hi[k] ? x : hi[k];
                }
            }
        }
        float *b = out + 8 * l;
        for (int k = 0; k < 3; ++k) {
            // rounded OUTWARD to float (nextafter on the double-to-float conversion's wrong side is covered by the margin: 2^-24 of a coordinate against 2^-9 of the scale)
            b[k] = ok ? static_cast<float>(lo[k] - M) : -inf;
            b[3 + k] = ok ? static_cast<float>(hi[k] + M) : inf;
        }
        b[6] = b[7] = 0.0f;
    }
}

inline void bounce_leaf_boxes(const float *tris, const size_t n_tris, const double scale, float *out) { bounce_group_boxes(tris, n_tris, scale, kLeafTris, out); }

constexpr double kBounceMarginScales = 0x1p-10;  // the table's margin in scene scales: eight times the float error a position can carry under the launch-time premise
constexpr double kBounceCameraScales = 64.0;     // ... which is: the camera (the first segment's origin) no further than this many scene scales from the world origin

// ---- the row boxes of the bounce rounds (round 8) ---------------------------------------------------------------------------------------------------------
// Nearly every packet of bounce rays leaves ONE triangle on one side (the headline frame: 96.8 %), and the shared leaf boxes cannot cull what such a packet walks:
// its rays start inside them, an EPSILON above a plane that most of the row's members lie in.  So every row 2 A + s gets boxes of its own, one per leaf, and a
// REFINED ROW beside them (same words, same stride as the table's): both keep of a member B only the part at height >= H0(B) above A's plane on side s (height:
// side * dot(x - v0_A, n_A) / |n_A| on the float record taken as exact, as bounce_row_word measures it).  Bit B of the refined row is set iff it is set in the
// table and some vertex of B reaches H0(B); the box of (row, leaf) bounds the polygons {x in B : height >= H0(B)} of those members (the triangle clipped at the
// plane, in double), widened by the leaf boxes' M and rounded to float; no such member: the empty box lo = +inf, hi = -inf, which a round never tests (the leaf's
// bits of the refined row are zero, and the walk looks at the bits first — the slab test itself is symmetric in lo and hi and cannot express "empty").
//
// H0 is derived.  eps = EPSILON, margin = 2^-10 scale (the table's), E' = scale + 2 eps.  A segment whose `leave` names (A, s) (rvpt_device.h: shade):
//   * starts at o = fma3(N', +-eps, pos), N' = the float unit normal of A (unit to 2^-22), pos = the accepted hit on A: on A's plane up to the float error of a
//     position, <= 2^-13 scale under the launch-time premise (camera within 64 scales; the table's proof budgets the same) — height(o) >= eps - 2^-13 scale -
//     2^-22 eps - 2^-23 E' (the fma's rounding of coordinates <= E');
//   * does not descend towards the plane, up to rounding: dot(d, N') >= -2^-18 |d| (Lambert: > 0; mirror: cos_in >= 0 with 2^-22 of error; refraction: eta 2^-22,
//     eta <= 16, else shade says "anywhere"); a point Y of the exact ray that an accepted pair needs lies within E_B of the scene, |Y - o| <= 4 E', so the
//     descent up to Y is <= 2^-16 E'.
//   So every point of the exact ray with t > 0 that matters has height >= eps - 2^-13 scale - 2^-15 E'.  The float test accepts (ray, B) only when such a point Y
//   lies within E_B = (33 * 2^-24 / kappa_B)(t + S) of a point X of B (rvpt_rect.h), and height is 1-Lipschitz: height(X) >= eps - 2^-13 scale - 2^-15 E' - E_B.
//   With t |d| <= 4 E' and S = |o|_1 + |v0 - o|_1 + |e0|_1 + |e1|_1 <= 6 E' + |e0|_1 + |e1|_1:  E_B <= (33 * 2^-24 / kappa_B)(10 E' + |e0|_1 + |e1|_1), computed per B.
//   H0(B) = eps - margin - 2^-14 E' - E_B  —  the whole margin where the proof needs an eighth of it, 2^-14 E' where it needs 2^-15: looser than necessary, provable.
//   X therefore lies in B's clipped polygon, and Y inside the polygon's bounds widened by E_B.  As for the leaf boxes the widening M = 2^-9 E' pays for E_B
//   (a member with E_B > 0.4 M — kappa_B near 2^-6 — breaks the premise) and for the slab test's own error, 2^-12 of the remaining 0.6 M.
// Premises, carried over from the table and the leaf boxes: A and B finite, non-degenerate, kappa >= 2^-6, a scene that has a scale; and E_B <= 0.4 M.  Where A
// fails, the row's boxes are the shared leaf boxes and its refined words the table's; where a member B fails, its leaf's box in that row is the shared leaf box
// and B's bit stays.  A positive H0 (scale < ~1.5 eps 2^10: the headline's is 3.2, H0 = +0.0016) drops the coplanar neighbours and A itself from the row; a scene
// far larger than EPSILON gets H0 ~ -margin and keeps only what the clipped boxes save.
// Checked like the table: tests/test_row_boxes.py (float64 restatement, GPU-free) and rvpt_hip_selftest_bounce_cull out[7] (accepted pairs that fail their row box
// or whose refined bit is cleared: 0).
constexpr double kRowSlackScales = 0x1p-14;

// ---- the TIGHT rule of the row boxes ----------------------------------------------------------------------------------------------------------------------
// The rule above spends eight times the slack its derivation asks for, and on the headline frame that slack is what the bounce rounds walk: the rays start at
// eps = 0.005 over the leaving plane, INSIDE boxes widened by M = 0.0063, and the coplanar neighbours whose corners rise 0.002 - 0.004 over that plane stay in the
// row (H0 = +0.0016).  The tight rule spends TWICE what the derivation asks for, term by term, and widens every member by what that member needs:
//   H0(B) = eps - margin / 4 - 2^-14 E' - E_B                     (the headline: +0.0039)
//   W_B   = 2.5 E_B + 2^-16 E'   around B's clipped polygon, per member, before the leaf's union (the leaf does not take one M)
// H0.  The derivation above holds as written, and nothing in it is particular to the old constants: height(o) >= eps - 2^-13 scale - 2^-22 eps - 2^-23 E' (the
//   accepted hit's position error under the launch-time premise of a camera within 64 scales, the unit normal's and the fma's rounding), the descent up to Y is
//   <= 2^-16 E', so every point of the exact ray with t > 0 that matters has height >= eps - 2^-13 scale - 2^-15 E' (2^-16 + 2^-22 + 2^-23 < 2^-15), and the X of B
//   that an accepted pair needs has height(X) >= eps - 2^-13 scale - 2^-15 E' - E_B.  margin / 4 = 2^-12 scale is twice the first term, 2^-14 E' twice the second;
//   E_B is the bound itself (rvpt_rect.h), taken once as above.  No term was found that the derivation misses: the divisor is 4, the largest power of two that
//   leaves a factor of two on the position error (8 would leave none).
// W_B.  X lies in B's clipped polygon {height >= H0(B)} and |Y - X| <= E_B, so Y lies inside the polygon's bounds widened by E_B.  What the widening pays besides:
//   the slab test's own error, <= 2^-21 (|b| + |o|) |inv| in t (leaf boxes, above), i.e. <= 2^-21 * 2 E' = 2^-20 E' in position along the axis — a sixteenth of the
//   2^-16 E' term; and the rounding of the box to float (to nearest, not outward): <= 2^-24 of a coordinate <= 2^-24 E'.  Needed: E_B + 2^-20 E' + 2^-24 E'; spent:
//   2.5 E_B + 2^-16 E', so E_B <= 0.4 W_B as the leaf boxes' proof has it, with 1.5 E_B and more than 7/8 of the 2^-16 E' left over.
// Premises: A and B finite, non-degenerate, kappa >= 2^-6, a scene that has a scale — as above, with the same fallbacks (A fails: the shared leaf boxes and the
//   table's words; B fails: its leaf's shared box in that row, and B's bit stays).  The premise E_B <= 0.4 M is NO LONGER NEEDED for a member's own widening — W_B
//   is made from E_B, whatever it is.  The rule still sends a member beyond it to the shared box and caps W_B at M (where E_B <= 0.4 M, M is enough by the old
//   rule's proof; the cap bites only for 0.4 M (1 - 2^-7) < E_B <= 0.4 M), for one reason only: with H0 no lower than the old rule's, every tight box then lies
//   inside the old rule's box of the same (row, leaf) and every tight row inside the old row — which the tests check, and which makes the old rule's selftest
//   and fuzz history evidence for the new one.
// Checked: tests/test_row_boxes_tight.py (float64 restatement, GPU-free), tests/test_row_boxes_tight_gpu.py (selftest out[7], bit-exact frames against the old rule).
struct RowRule {
    double margin_div;    // H0 spends margin / margin_div
    double slack_scales;  // ... and slack_scales * E'
    bool per_member;      // the widening: true = W_B = kRowWidenEB * E_B + kRowWidenScales * E' (at most M) around every member's clipped part; false = one M around the leaf's union
};
constexpr double kRowWidenEB = 2.5, kRowWidenScales = 0x1p-16;
constexpr RowRule kRowRuleShipped = {1.0, kRowSlackScales, false};  // (round 8; RVPT_HIP_PACKETS_ROW_RULE=0 in the laboratory build)
constexpr RowRule kRowRuleTight = {4.0, kRowSlackScales, true};

// One word w of the refined row `row` (returned) and the boxes of its 32 / kLeafTris leaves (boxes_out: 8 floats each — lo.xyz, hi.xyz, 0, 0).  prep, n, row, w:
// bounce_row_word's; scale = bounce_scene_scale; leaf_boxes = bounce_leaf_boxes' array, padded to whole words (leaf 32 / kLeafTris * w + k at 8 floats each)
RV_HD uint32_t bounce_row_boxes_word_rule(const RowRule rule, const float *prep, const uint32_t n, const uint32_t row, const uint32_t w, const double scale, const float *leaf_boxes,
                                          float *boxes_out)
{
    constexpr uint32_t kPerWord = 32u / kLeafTris;
    const double eps = static_cast<double>(kEpsilon);
    const double margin = kBounceMarginScales * scale;
    const double Es = scale + 2.0 * eps;
    const double M = kLeafBoxMarginScales * (scale + 2.0 * 0.005);  // bounce_group_boxes' M
    const double Wleaf = rule.per_member ? 0.0 : M;                 // (x - 0.0 == x: one body serves both forms, and the old rule's output stays byte for byte)
    const uint32_t bits = bounce_row_word(prep, n, row, w, margin);
    const uint32_t A = row >> 1;
    const double side = (row & 1u) ? -1.0 : 1.0;
    const float *a = prep + 16u * A;
    const double av0[3] = {a[0], a[1], a[2]}, an[3] = {a[3], a[4], a[5]}, ae0[3] = {a[6], a[7], a[8]}, ae1[3] = {a[9], a[10], a[11]};
    const double nn = __builtin_sqrt(an[0] * an[0] + an[1] * an[1] + an[2] * an[2]);
    bool a_ok;
    {
        const double a00 = ae1[0] * ae1[0] + ae1[1] * ae1[1] + ae1[2] * ae1[2], a11 = ae0[0] * ae0[0] + ae0[1] * ae0[1] + ae0[2] * ae0[2];
        const double a01 = ae0[0] * ae1[0] + ae0[1] * ae1[1] + ae0[2] * ae1[2];
        a_ok = (a00 * a11 - a01 * a01) >= 0x1p-6 * (a00 * a11) && a00 * a11 > 0.0 && nn > 0.0 && margin > 0.0;
        for (int k = 0; k < 3; ++k) a_ok = a_ok && (av0[k] - av0[k] == 0.0) && (an[k] - an[k] == 0.0);
    }
    const float inf = __builtin_inff();
    uint32_t refined = 0u;
    for (uint32_t k = 0; k < kPerWord; ++k) {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        bool shared = !a_ok, any = false;
        for (uint32_t b = kLeafTris * k; b < kLeafTris * (k + 1u); ++b) {
            const uint32_t B = 32u * w + b;
            if (B >= n) break;
            if (((bits >> b) & 1u) == 0u) continue;
            refined |= 1u << b;
            if (!a_ok) continue;
            const float *q = prep + 16u * B;
            const double v0[3] = {q[0], q[1], q[2]}, e0[3] = {q[6], q[7], q[8]}, e1[3] = {q[9], q[10], q[11]};
            const double a00 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], a11 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2];
            const double a01 = e0[0] * e1[0] + e0[1] * e1[1] + e0[2] * e1[2];
            const double kappa = (a00 * a11 - a01 * a01) / (a00 * a11);
            auto abs1 = [](const double *x) { return __builtin_fabs(x[0]) + __builtin_fabs(x[1]) + __builtin_fabs(x[2]); };
            const double EB = (33.0 * 0x1p-24 / kappa) * (10.0 * Es + abs1(e0) + abs1(e1));
            double p[3][3], h[3];
            bool b_ok = kappa >= 0x1p-6 && a00 * a11 > 0.0 && EB <= 0.4 * M;  // (NaN: false)
            for (int v = 0; v < 3; ++v) {
                for (int c = 0; c < 3; ++c) p[v][c] = v0[c] + (v == 1 ? e0[c] : (v == 2 ? e1[c] : 0.0));
                h[v] = side * ((p[v][0] - av0[0]) * an[0] + (p[v][1] - av0[1]) * an[1] + (p[v][2] - av0[2]) * an[2]) / nn;
                b_ok = b_ok && (h[v] - h[v] == 0.0) && (p[v][0] - p[v][0] == 0.0) && (p[v][1] - p[v][1] == 0.0) && (p[v][2] - p[v][2] == 0.0);
            }
            if (!b_ok) {  // a premise fails for this member: it stays, and its leaf keeps the shared box in this row
                shared = true;
                continue;
            }
            const double H0 = eps - margin / rule.margin_div - rule.slack_scales * Es - EB;
            const double WB = kRowWidenEB * EB + kRowWidenScales * Es;
            const double W = rule.per_member ? (WB < M ? WB : M) : 0.0;
            const bool up[3] = {h[0] >= H0, h[1] >= H0, h[2] >= H0};
            if (!(up[0] || up[1] || up[2])) {  // wholly below H0: no segment that leaves (A, s) is accepted by B
                refined &= ~(1u << b);
                continue;
            }
            any = true;
            for (int v = 0; v < 3; ++v) {
                const int u = v == 2 ? 0 : v + 1;
                if (up[v])
                    for (int c = 0; c < 3; ++c) lo[c] = p[v][c] - W < lo[c] ? p[v][c] - W : lo[c], hi[c] = p[v][c] + W > hi[c] ? p[v][c] + W : hi[c];
                if (up[v] != up[u]) {  // the edge v -> u crosses the plane height = H0 (h[u] != h[v])
                    const double s = (H0 - h[v]) / (h[u] - h[v]);
                    for (int c = 0; c < 3; ++c) {
                        const double x = p[v][c] + s * (p[u][c] - p[v][c]);
                        lo[c] = x - W < lo[c] ? x - W : lo[c], hi[c] = x + W > hi[c] ? x + W : hi[c];
                    }
                }
            }
        }
        float *o = boxes_out + 8u * k;
        const float *sb = leaf_boxes + 8u * (kPerWord * w + k);
        for (int c = 0; c < 3; ++c) {
            o[c] = shared ? sb[c] : (any ? static_cast<float>(lo[c] - Wleaf) : inf);
            o[3 + c] = shared ? sb[3 + c] : (any ? static_cast<float>(hi[c] + Wleaf) : -inf);
        }
        o[6] = o[7] = 0.0f;
    }
    return refined;
}

// the rule of round 8: {the whole margin, 2^-14 E', one M around the leaf's union}
RV_HD uint32_t bounce_row_boxes_word(const float *prep, const uint32_t n, const uint32_t row, const uint32_t w, const double scale, const float *leaf_boxes, float *boxes_out)
{
    return bounce_row_boxes_word_rule(kRowRuleShipped, prep, n, row, w, scale, leaf_boxes, boxes_out);
}

// ---- the ROW CAPS of the bounce rounds -------------------------------------------------------------------------------------------------------------------
// What is left in the tight rows are mostly A's near-coplanar neighbours, a few degrees off A's plane.  To reach one a ray must leave A at a LOW ELEVATION, and a
// Lambert direction seldom does: P(sin elevation < s) = s^2.  So every row 2 A + s gets one number K, an upper bound of sin^2 of the elevation over A's plane at
// which a segment that leaves (A, s) can still be accepted by ANY member of the row, and a packet whose rays all leave (A, s) above it walks nothing at all.
//
// The cap.  n^ = A's exact unit normal turned to side s, height h(x) = dot(x - v0_A, n^) as above, eps, margin, E', E_B as above.  A segment whose `leave` names
//   (A, s) starts at o with h(o) >= h_o = eps - 2^-13 scale - 2^-15 E', and every point of the exact ray with t > 0 that matters has height >= h_o (the row boxes'
//   derivation: it needs `leave`'s premise that the ray does not descend by more than 2^-18 |d|).  The float test accepts (ray, B) only when a point Y = o + t d,
//   t > 0, of the exact ray lies within E_B of a point X of B; so h(X) >= h_o - E_B and h(X) >= H0(B) (the tight rule's): X lies in
//     P_B = B clipped at height >= max(H0(B), h_o - E_B)          (empty: no segment is accepted, cap 0).
//   Rise:  t dot(d, n^) = h(Y) - h(o) <= h(X) + E_B - h_o.
//   Run:   o projects within rho_A of triangle A.  o = fma3(N', +-eps, pos); pos is the float position of the accepted hit on A: the exact ray's point lies within
//     E_A of a point of A (the float test's bound (33 eps / kappa_A)(t + S), rvpt_rect.h; the segment that hit A may be a camera ray, whose origin lies up to 64
//     scales out under the launch-time premise: t |d| <= 113 scales, S <= 390 scales + the edges, so E_A = (33 eps / kappa_A)(512 E' + |e0|_1 + |e1|_1)), pos
//     within 2^-13 scale of that point (the position error the table budgets under the same premise), the fma rounds coordinates <= E' (sqrt(3) 2^-24 E'), and eps N' leaves n^'s line by <= 2^-21 eps.  Projection onto A's
//     plane is 1-Lipschitz:  rho_A = E_A + 2^-12 scale + 2^-20 E'  (twice the position term, more than eight times the others).  For an edge line k of A (through
//     a_k, outward in-plane unit normal m_k, s_k(x) = dot(x - a_k, m_k) <= 0 on A):  s_k(o) <= rho_A, s_k(Y) >= s_k(X) - E_B, so
//     t dot(d, m_k) >= s_k(X) - E_B - rho_A.
//   Where that is > 0 at every vertex of P_B (edge k SEPARATES A from P_B), dot(d, n^) / dot(d, m_k) <= (h(X) + E_B - h_o) / (s_k(X) - E_B - rho_A), a ratio of two
//   affine functions with a positive denominator over a convex polygon: largest at a vertex.  tan cap_B = min over separating k of max over the vertices; no such
//   edge, or A or B failing a premise: +inf.  The premises are the row boxes' — finite, non-degenerate, kappa >= 2^-6, a scene that has a scale — without E_B <= 0.4 M:
//   every step above takes E_B as it is, and the clip that counts, h_o - E_B, is proved here and not taken from the row (a member the tight rule keeps only because
//   its E_B is large is clipped at its own, lower, height).  dot(d, m_k) <= sqrt(|d|^2 - dot(d, n^)^2), hence for an accepted pair
//     dot(d, n^) <= 0   or   dot(d, n^)^2 <= sin^2(cap_B) |d|^2,          sin^2 = tan^2 / (1 + tan^2).
// The float evaluation (rvpt_packets.hip): c = dot(d, sN') in float, sN' the float unit normal the table holds, dd = dot(d, d); a lane is OUT OF REACH when
//   c > 0 && c * c > K * dd.  |sN' - n^| <= 2^-21 (bounce_row_cap_normal_ok checks it in double against the very floats, else K = +inf), the dot's three products
//   and two sums carry <= 3 * 2^-24 |d| |N'|: |c - dot(d, n^)| <= 2^-20 |d|.  dd and the two products of the compare carry 2^-22 and 2^-24 relative.  So the compare
//   implies dot(d, n^) > (sqrt(K) (1 - 2^-21) - 2^-20) |d|, which is >= sin(cap) |d| for sqrt(K) = max(sin(cap) (1 + 2^-20) + 2^-19, 2^-18); K goes up by 2^-22
//   more before it is rounded to float (to nearest: 2^-24).  The floor keeps every lane with c <= 2^-18 |d| on the walk (what a descent by rounding looks like);
//   |d|^2 >= 2^-16 for every direction `leave` vouches for, so neither product underflows; K = +inf says "no cap", and a NaN anywhere makes the compare false.
// K_row = the largest K of the row's members, K_leaf the same per leaf of kLeafTris triangles.  The caps name no box and no refined bit: they hold for the table's
// row (a member the tight rule drops has an empty P_B), whichever rule made the boxes.
// Checked: tests/test_row_caps.py (float64 restatement, brute-force soundness, simulated paths; GPU-free), tests/test_row_caps_gpu.py (bit-exact frames against
// K = +inf; rvpt_hip_selftest_bounce_cull out[7] counts accepted pairs the row cap declares out of reach: 0).
constexpr double kRowCapFloor = 0x1p-18;  // of sqrt(K)

RV_HD float bounce_row_cap_k(const double tan_cap)
{
    if (!(tan_cap < 1e300)) return __builtin_inff();  // (+inf or NaN: no cap)
    const double s = tan_cap / __builtin_sqrt(1.0 + tan_cap * tan_cap);
    double r = s * (1.0 + 0x1p-20) + 0x1p-19;
    r = r > kRowCapFloor ? r : kRowCapFloor;
    return static_cast<float>(r * r * (1.0 + 0x1p-22));
}

// is the float unit normal un (FrameParams::unit_n of A, not yet turned to the side) within 2^-21 of the exact one of A's record?
RV_HD bool bounce_row_cap_normal_ok(const float *prep, const uint32_t A, const float *un)
{
    const float *a = prep + 16u * A;
    const double an[3] = {a[3], a[4], a[5]};
    const double nn = __builtin_sqrt(an[0] * an[0] + an[1] * an[1] + an[2] * an[2]);
    double d2 = 0.0;
    for (int c = 0; c < 3; ++c) d2 += (an[c] / nn - un[c]) * (an[c] / nn - un[c]);
    return d2 <= 0x1p-42;  // (NaN: false)
}

// K_row of row 2 A + s (returned) and, where k_leaf is given, K_leaf of its 32 / kLeafTris * words leaves.  prep, n, scale: bounce_row_boxes_word_rule's
RV_HD float bounce_row_caps_row(const float *prep, const uint32_t n, const uint32_t row, const uint32_t words, const double scale, float *k_leaf)
{
    constexpr uint32_t kPerWord = 32u / kLeafTris;
    const double eps = static_cast<double>(kEpsilon);
    const double margin = kBounceMarginScales * scale;
    const double Es = scale + 2.0 * eps;
    const double inf = static_cast<double>(__builtin_inff());
    const uint32_t A = row >> 1;
    const double side = (row & 1u) ? -1.0 : 1.0;
    const float *a = prep + 16u * A;
    const double av0[3] = {a[0], a[1], a[2]}, an[3] = {a[3], a[4], a[5]}, ae0[3] = {a[6], a[7], a[8]}, ae1[3] = {a[9], a[10], a[11]};
    const double nn = __builtin_sqrt(an[0] * an[0] + an[1] * an[1] + an[2] * an[2]);
    auto abs1 = [](const double *x) { return __builtin_fabs(x[0]) + __builtin_fabs(x[1]) + __builtin_fabs(x[2]); };
    bool a_ok;
    double rhoA;
    {
        const double a00 = ae1[0] * ae1[0] + ae1[1] * ae1[1] + ae1[2] * ae1[2], a11 = ae0[0] * ae0[0] + ae0[1] * ae0[1] + ae0[2] * ae0[2];
        const double a01 = ae0[0] * ae1[0] + ae0[1] * ae1[1] + ae0[2] * ae1[2];
        a_ok = (a00 * a11 - a01 * a01) >= 0x1p-6 * (a00 * a11) && a00 * a11 > 0.0 && nn > 0.0 && margin > 0.0;
        for (int k = 0; k < 3; ++k) a_ok = a_ok && (av0[k] - av0[k] == 0.0) && (an[k] - an[k] == 0.0);
        const double kappaA = (a00 * a11 - a01 * a01) / (a00 * a11);
        const double EA = (33.0 * 0x1p-24 / kappaA) * (512.0 * Es + abs1(ae0) + abs1(ae1));  // (the segment that hit A may have come from the camera)
        rhoA = EA + 0x1p-12 * scale + 0x1p-20 * Es;
        a_ok = a_ok && (rhoA - rhoA == 0.0);
    }
    const double h_o = eps - 0x1p-13 * scale - 0x1p-15 * Es;
    // A's three edge lines: a point a_k and the outward in-plane unit normal m_k
    double ea[3][3], em[3][3];
    for (int k = 0; k < 3; ++k) {
        double pa[3], pb[3], pc[3];
        for (int c = 0; c < 3; ++c) {
            const double v[3] = {av0[c], av0[c] + ae0[c], av0[c] + ae1[c]};
            pa[c] = v[k], pb[c] = v[k == 2 ? 0 : k + 1], pc[c] = v[k == 0 ? 2 : k - 1];
        }
        const double e[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]};
        double m[3] = {e[1] * an[2] - e[2] * an[1], e[2] * an[0] - e[0] * an[2], e[0] * an[1] - e[1] * an[0]};
        const double len = __builtin_sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
        a_ok = a_ok && len > 0.0 && (len - len == 0.0);
        const double inward = (pc[0] - pa[0]) * m[0] + (pc[1] - pa[1]) * m[1] + (pc[2] - pa[2]) * m[2];
        for (int c = 0; c < 3; ++c) ea[k][c] = pa[c], em[k][c] = (inward > 0.0 ? -m[c] : m[c]) / len;
    }
    double row_tan = 0.0;
    for (uint32_t w = 0; w < words; ++w) {
        const uint32_t bits = bounce_row_word(prep, n, row, w, margin);
        for (uint32_t k = 0; k < kPerWord; ++k) {
            double leaf_tan = 0.0;
            for (uint32_t b = kLeafTris * k; b < kLeafTris * (k + 1u); ++b) {
                const uint32_t B = 32u * w + b;
                if (B >= n) break;
                if (((bits >> b) & 1u) == 0u) continue;
                if (!a_ok) {
                    leaf_tan = inf;
                    continue;
                }
                const float *q = prep + 16u * B;
                const double v0[3] = {q[0], q[1], q[2]}, e0[3] = {q[6], q[7], q[8]}, e1[3] = {q[9], q[10], q[11]};
                const double a00 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], a11 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2];
                const double a01 = e0[0] * e1[0] + e0[1] * e1[1] + e0[2] * e1[2];
                const double kappa = (a00 * a11 - a01 * a01) / (a00 * a11);
                const double EB = (33.0 * 0x1p-24 / kappa) * (10.0 * Es + abs1(e0) + abs1(e1));
                double p[3][3], h[3];
                bool b_ok = kappa >= 0x1p-6 && a00 * a11 > 0.0 && (EB - EB == 0.0);  // (the row boxes' premises but E_B <= 0.4 M, which nothing here needs; NaN: false)
                for (int v = 0; v < 3; ++v) {
                    for (int c = 0; c < 3; ++c) p[v][c] = v0[c] + (v == 1 ? e0[c] : (v == 2 ? e1[c] : 0.0));
                    h[v] = side * ((p[v][0] - av0[0]) * an[0] + (p[v][1] - av0[1]) * an[1] + (p[v][2] - av0[2]) * an[2]) / nn;
                    b_ok = b_ok && (h[v] - h[v] == 0.0) && (p[v][0] - p[v][0] == 0.0) && (p[v][1] - p[v][1] == 0.0) && (p[v][2] - p[v][2] == 0.0);
                }
                if (!b_ok) {
                    leaf_tan = inf;
                    continue;
                }
                const double H0 = eps - margin / kRowRuleTight.margin_div - kRowRuleTight.slack_scales * Es - EB;
                const double Hc = H0 > h_o - EB ? H0 : h_o - EB;
                // the vertices of P_B: the corners at height >= Hc and the points where an edge crosses it
                double x[6][3], xh[6];
                int nx = 0;
                const bool up[3] = {h[0] >= Hc, h[1] >= Hc, h[2] >= Hc};
                for (int v = 0; v < 3; ++v) {
                    const int u = v == 2 ? 0 : v + 1;
                    if (up[v]) {
                        for (int c = 0; c < 3; ++c) x[nx][c] = p[v][c];
                        xh[nx++] = h[v];
                    }
                    if (up[v] != up[u]) {
                        const double s = (Hc - h[v]) / (h[u] - h[v]);
                        for (int c = 0; c < 3; ++c) x[nx][c] = p[v][c] + s * (p[u][c] - p[v][c]);
                        xh[nx++] = Hc;
                    }
                }
                if (nx == 0) continue;  // empty: cap 0
                double cap = inf;
                for (int e = 0; e < 3; ++e) {
                    bool separates = true;
                    double worst = 0.0;
                    for (int i = 0; i < nx; ++i) {
                        const double den = (x[i][0] - ea[e][0]) * em[e][0] + (x[i][1] - ea[e][1]) * em[e][1] + (x[i][2] - ea[e][2]) * em[e][2] - EB - rhoA;
                        const double num = xh[i] + EB - h_o;
                        separates = separates && den > 0.0;  // (NaN: false)
                        const double r = (num > 0.0 ? num : 0.0) / den;
                        worst = r > worst ? r : worst;
                    }
                    if (separates && worst < cap) cap = worst;
                }
                leaf_tan = cap > leaf_tan ? cap : leaf_tan;
            }
            if (k_leaf) k_leaf[kPerWord * w + k] = bounce_row_cap_k(leaf_tan);
            row_tan = leaf_tan > row_tan ? leaf_tan : row_tan;
        }
    }
    return bounce_row_cap_k(row_tan);
}

}  // namespace rv
