// rvpt_packets.h — the packet form of the LDS-resident brute-force frame kernel (rvpt_packets.hip)
#pragma once

#include "rvpt_kernels.h"
#include "rvpt_math.h"

namespace rv {

constexpr uint32_t kPacketQueueWords = 18;     // words of a parked path; a wave's queue holds 64 of them (4.5 KiB)
constexpr uint32_t kPacketQueueWordsAA1 = 15;  // ... one sample per pixel: without the pixel's sum of finished samples (trace_brute_packets_aa1)

// lean configuration only (Kajiya in all quadrants, pinhole camera, max_bounces >= 1), scene + materials resident in LDS
__global__ void trace_brute_packets(const FrameParams p);
__global__ void trace_brute_packets_aa1(const FrameParams p);  // aa == 1: 15-word queue entries, six work-groups per CU
__global__ void trace_brute_packets_culls(const FrameParams p);      // the same two for launches that ride with all three exact culls and whole-block work plans
__global__ void trace_brute_packets_aa1_culls(const FrameParams p);  // (the walks without a cull are not in them; nor the interleaved claim order of short launches:)
__global__ void trace_brute_packets_culls_order(const FrameParams p);
__global__ void trace_brute_packets_aa1_culls_order(const FrameParams p);
// The LISTED instance (batched launches of a still camera, one sample per pixel): the claims count only the blocks of a frame that are not SKY (sky_blocks below), 64
// work items per block of `list` (ascending frame-local block indices) per frame — n_listed_frame items per frame; blend_accumulate_sky makes the sky blocks' samples
// FRAME RUNS (run_frames = F > 0, trace_brute_packets_aa1_culls_listed_runs): the items are ordered by GROUP of F consecutive frames (the last group may be shorter),
// then list position, then frame within the group, so that a block's F camera rounds follow each other (F = 16: two 512-item claims) and a wave does what depends
// on the camera and the block alone — the pixel coordinates, their hash, the candidate triangles — once per run (listed_item below; packets_body: the run header)
struct ListedWork {
    const uint2 *list;        // per listed block: (frame-local block index, pixel coordinates of its first item as gx0 | gy0 << 16)
    uint32_t n_listed_frame;  // 64 x the blocks of the list
    FastDiv div_listed_frame;
    uint32_t run_frames;      // F; 0 = frame-major order (items ordered by frame, then list position)
    uint32_t n_blocks;        // the blocks of the list
    uint32_t n_full_groups;   // frames of the launch / F
    uint32_t last_frames;     // frames of the launch % F: the frames of the short last group (0: there is none)
    FastDiv div_group, div_run, div_last;  // by F * n_blocks (the blocks' items of a whole group), by F and by max(last_frames, 1)
};
// host side of the above for a launch of n_frames frames over a list of n_blocks blocks
inline void listed_runs_make(ListedWork &w, const uint32_t n_blocks, const uint32_t n_frames, const uint32_t run_frames)
{
    w.run_frames = run_frames;
    w.n_blocks = n_blocks;
    w.n_full_groups = run_frames ? n_frames / run_frames : 0u;
    w.last_frames = run_frames ? n_frames % run_frames : 0u;
    w.div_group = fast_div_make(run_frames * n_blocks);
    w.div_run = fast_div_make(run_frames);
    w.div_last = fast_div_make(w.last_frames ? w.last_frames : 1u);
}
// block-item k of a launch in frame-run order (item index >> 6) -> the frame offset in the launch and the position in the list
RV_HD void listed_item(const ListedWork &w, const uint32_t k, uint32_t &frame, uint32_t &pos)
{
    const uint32_t g = fast_div(k, w.div_group);
    const uint32_t r = k - g * (w.run_frames * w.n_blocks);
    const bool last = g >= w.n_full_groups;  // (the short group: last_frames * n_blocks < F * n_blocks items, all of them with g = n_full_groups)
    pos = fast_div(r, last ? w.div_last : w.div_run);
    frame = g * w.run_frames + (r - pos * (last ? w.last_frames : w.run_frames));
}
__global__ void trace_brute_packets_aa1_culls_listed(const FrameParams p, const ListedWork w);
__global__ void trace_brute_packets_aa1_culls_listed_runs(const FrameParams p, const ListedWork w);
#if RVPT_HIP_LAB
// diagnostics (rvpt_hip_selftest_pretest): per element, bit 0 = the division-free pre-test of a camera round lets the pair through, bit 1 = the
// quotient's own condition 0 < t < closest holds; the numerator goes through the camera record's rule (not safe -> NaN -> always through)
__global__ void selftest_camera_pretest(const float *__restrict__ a, const float *__restrict__ den, const float *__restrict__ closest,
                                        unsigned char *__restrict__ out, uint32_t n);
#endif

// the screen rectangles of the prepared triangles for the camera of `p` (rvpt_rect.h): rects[i] = (x0 | x1 << 16, y0 | y1 << 16); one thread per triangle
__global__ void camera_rects(const FrameParams p, uint2 *__restrict__ rects, float4 *__restrict__ records);  // (+ the camera records, 16 B per triangle, or nullptr)
// the SKY blocks of a frame for the same camera: bit b of sky_bits (ceil(n_blocks / 32) words) = no rectangle holds the frame's 16 x 4 block b (work items 64 b ..) or
// the block lies wholly outside the image; one thread per block, 256 per work-group
__global__ void sky_blocks(const FrameParams p, const uint2 *__restrict__ rects, uint32_t n_blocks, uint32_t *__restrict__ sky_bits);
// ... and the blocks that are not, in ascending order, each with the pixel coordinates of its first item (ListedWork::list), and their count: ONE work-group of 1024 threads
__global__ void sky_list(const FrameParams p, const uint32_t *__restrict__ sky_bits, uint32_t n_blocks, uint2 *__restrict__ list, uint32_t *__restrict__ count);
// the bounce cull's table for `n` prepared triangles: out[(2 A + s) * words + w] bit b = 0 only when triangle B = 32 w + b lies wholly behind the plane of A as
// seen from side s (s = 0: the side A's normal cross(e0, e1) points to), by more than `margin`, and both triangles are well shaped; bits >= n are 0
__global__ void bounce_visibility(const float4 *__restrict__ prep, uint32_t n, double margin, uint32_t words, uint32_t stride, uint32_t *__restrict__ out);
// the row boxes of the same table (rvpt_vis.h: bounce_row_boxes_word): refined[(2 A + s) * stride + w] and the 32 / kLeafTris boxes of that word at
// boxes[8 * ((2 A + s) * (32 / kLeafTris) * words + (32 / kLeafTris) * w)]; leaf_boxes: bounce_leaf_boxes' array padded to whole words; one thread per (row, word);
// tight != 0: the tight rule (kRowRuleTight), 0: round 8's (kRowRuleShipped)
__global__ void bounce_row_boxes(const float4 *__restrict__ prep, uint32_t n, double scale, uint32_t words, uint32_t stride, const float *__restrict__ leaf_boxes,
                                 uint32_t *__restrict__ refined, float *__restrict__ boxes, uint32_t tight);
// the row caps of the same table (rvpt_vis.h: bounce_row_caps_row): caps[2 A + s] = (unit_n[A] turned to side s, K_row); enabled == 0: every K = +inf (no round skips);
// one thread per row
__global__ void bounce_row_caps(const float4 *__restrict__ prep, const float4 *__restrict__ unit_n, uint32_t n, double scale, uint32_t words, uint32_t enabled,
                                float4 *__restrict__ caps);
#if RVPT_HIP_LAB
// diagnostics (rvpt_hip_selftest_bounce_cull): every pixel x n_samples paths traced against EVERY triangle; on segments that leave a triangle, out[0] += pairs the
// float test accepts with the interval wide open, out[1] += those whose triangle is NOT in the row of where the segment leaves from (must stay 0), out[2] += those whose
// ray fails the slab test of the triangle's leaf box (must stay 0), out[3] / out[4] += (ray, leaf box) pairs tested / passed, out[5] += those whose bit is cleared in
// the refined row of where the segment leaves from, whose ray fails the slab test of that row's box of the triangle's leaf, or whose segment the row cap of where it
// leaves from declares out of reach (row boxes and row caps; must stay 0)
__global__ void selftest_bounce_cull(const FrameParams p, uint32_t n_samples, unsigned long long *__restrict__ out);
// diagnostics (rvpt_hip_selftest_camera_rects): every pixel of the image x n_samples jittered camera rays x every triangle through the float test with
// an open interval; out[0] += accepted pairs, out[1] += accepted pairs whose block lies OUTSIDE the triangle's rectangle (must stay 0),
// out[2] += (16 x 4 block, triangle) pairs whose rectangle holds the block, out[3] += all such pairs
__global__ void selftest_camera_rects(const FrameParams p, const uint2 *__restrict__ rects, uint32_t n_samples, unsigned long long *__restrict__ out);
#endif

}  // namespace rv
