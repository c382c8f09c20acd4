// rvpt_refit.hip — the geometry update's kernels (rvpt_hip_upload_scene's update form: same topology, moved vertices): the boxes of the tree recomputed on the
// device.  Not frame kernels: this file is outside build.py's KERNEL_SOURCES, so the frame kernels' identity (kernel_sha) and the profiles stamped with it stand.
//
// min / max of floats is exact and order-independent, so the result is THE refit of the tree (rvpt_amd/scene.py: refit_bvh is the same in numpy), not an
// approximation of it.  (Only the sign of a zero bound may differ between two orders; a slab test cannot tell: (+-0 - o) * inv compares equal.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvpt_refit.h"

namespace rv {

// One launch per level of the breadth-first device layout, deepest first, in stream order: a level is the index range [begin, end), children have higher
// indices than their parent and lie on deeper levels, so every box a thread reads was written by an earlier launch.  No atomics, no waiting on another
// work-group.  A node = two quads: (first, count, minx, maxx), (miny, maxy, minz, maxz); only the six bounds are written.
__global__ void refit_level(float4 *__restrict__ nodes, uint32_t begin, uint32_t end, uint32_t n_nodes, const float4 *__restrict__ tris, uint32_t n_tris)
{
    const uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= end || i >= n_nodes) return;
    const float4 head = nodes[2 * i];
    const uint32_t first = __float_as_uint(head.x), count = __float_as_uint(head.y);
    float lo[3], hi[3];
    if (count > 0) {  // a leaf: its triangles' nine coordinates each
        if (first >= n_tris || count > n_tris - first) return;  // (upload_scene validated the ranges; a stray word must not become an address)
        const float4 a0 = tris[4 * first];
        lo[0] = hi[0] = a0.x, lo[1] = hi[1] = a0.y, lo[2] = hi[2] = a0.z;
        for (uint32_t t = first; t < first + count; ++t)
            for (uint32_t v = 0; v < 3; ++v) {
                const float4 p = tris[4 * t + v];
                lo[0] = fminf(lo[0], p.x), hi[0] = fmaxf(hi[0], p.x);
                lo[1] = fminf(lo[1], p.y), hi[1] = fmaxf(hi[1], p.y);
                lo[2] = fminf(lo[2], p.z), hi[2] = fmaxf(hi[2], p.z);
            }
    } else {  // an inner node: its two children, refitted by the launch before this one
        if (first <= i || first >= n_nodes - 1u) return;  // (children lie behind their parent in this layout)
        const float4 l0 = nodes[2 * first], l1 = nodes[2 * first + 1], r0 = nodes[2 * first + 2], r1 = nodes[2 * first + 3];
        lo[0] = fminf(l0.z, r0.z), hi[0] = fmaxf(l0.w, r0.w);
        lo[1] = fminf(l1.x, r1.x), hi[1] = fmaxf(l1.y, r1.y);
        lo[2] = fminf(l1.z, r1.z), hi[2] = fmaxf(l1.w, r1.w);
    }
    nodes[2 * i] = make_float4(head.x, head.y, lo[0], hi[0]);
    nodes[2 * i + 1] = make_float4(lo[1], hi[1], lo[2], hi[2]);
}

// ... then the 4-wide form: slot s of wide node w holds a copy of the box of binary node map[4 w + s] (build_wide_nodes' grouping, kept from the full upload;
// 0xFFFFFFFF = unused slot).  One thread per slot; heads and padding are not touched.  Wide node = minx[4] maxx[4] miny[4] maxy[4] minz[4] maxz[4] head[4] pad[4].
__global__ void refit_wide_gather(float *__restrict__ wide, const uint32_t *__restrict__ map, uint32_t n_slots, const float4 *__restrict__ nodes, uint32_t n_nodes)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_slots) return;
    const uint32_t b = map[t];
    if (b >= n_nodes) return;
    const float4 q0 = nodes[2 * b], q1 = nodes[2 * b + 1];
    float *q = wide + static_cast<size_t>(t >> 2) * 32u + (t & 3u);
    q[0] = q0.z, q[4] = q0.w, q[8] = q1.x, q[12] = q1.y, q[16] = q1.z, q[20] = q1.w;
}

}  // namespace rv
