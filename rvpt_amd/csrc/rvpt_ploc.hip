// rvpt_ploc.hip — the PLOC build form's kernels (rvpt_build.h holds the specification of the tree): parallel locally-ordered clustering over the leaf order the
// LBVH stages 1-3 leave behind, then the finished tree laid out level by level in the breadth-first device layout.  Not frame kernels: this file is outside
// build.py's KERNEL_SOURCES, so the frame kernels' identity (kernel_sha) and the profiles stamped with it stand.
//
// While more than kPlocTailClusters clusters are left an iteration is four launches (nearest neighbour, keep flags, rocPRIM's scan, scatter) and the host reads
// the new count, one word; the rest — most of the iterations, all of them on small arrays — run in ONE work-group that loops in LDS (ploc_tail).  Every kernel
// is one thread per cluster with its bounds checked against the capacity of what it writes; no kernel waits on another work-group.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <rocprim/device/device_scan.hpp>

#include "rvpt_build.h"

namespace rv {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;

inline uint32_t blocks_for(uint32_t n) { return (n + kThreads - 1u) / kThreads; }

struct Box {
    float lo[3], hi[3];
};

// d(i, j): the half-area of the union box in double, left to right, no contraction; not finite -> +inf
__device__ inline double union_half_area(const float *alo, const float *ahi, const float *blo, const float *bhi)
{
    double e[3];
    for (int ax = 0; ax < 3; ++ax) e[ax] = __dsub_rn(static_cast<double>(fmaxf(ahi[ax], bhi[ax])), static_cast<double>(fminf(alo[ax], blo[ax])));
    const double d = __dadd_rn(__dadd_rn(__dmul_rn(e[0], e[1]), __dmul_rn(e[1], e[2])), __dmul_rn(e[2], e[0]));
    return (d - d == 0.0) ? d : __longlong_as_double(0x7FF0000000000000ll);  // (inf - inf and NaN - NaN are NaN)
}

// the smaller of two candidates of cluster i by (d, i xor j, min(i, j))
__device__ inline bool better(double d, uint32_t i, uint32_t j, double best_d, uint32_t best_j)
{
    if (best_j == kNone) return true;
    if (d != best_d) return d < best_d;
    const uint32_t x = i ^ j, bx = i ^ best_j;
    if (x != bx) return x < bx;
    return min(i, j) < min(i, best_j);
}

// one cluster per sorted triangle: the exact min / max of its nine vertex coordinates (a NaN takes no part), provisional node = its sorted position
__global__ void ploc_init(const float4 *__restrict__ tris, uint32_t n, Box *__restrict__ boxes, uint32_t *__restrict__ ids)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = tris[4u * i], b = tris[4u * i + 1u], c = tris[4u * i + 2u];
    Box o;
    o.lo[0] = fminf(fminf(a.x, b.x), c.x), o.hi[0] = fmaxf(fmaxf(a.x, b.x), c.x);
    o.lo[1] = fminf(fminf(a.y, b.y), c.y), o.hi[1] = fmaxf(fmaxf(a.y, b.y), c.y);
    o.lo[2] = fminf(fminf(a.z, b.z), c.z), o.hi[2] = fmaxf(fmaxf(a.z, b.z), c.z);
    boxes[i] = o;
    ids[i] = i;
}

// nn[i] over the m clusters: a work-group stages the boxes of its window and kPlocRadius on either side in LDS (6 x 288 floats), every lane then evaluates its
// <= 2 kPlocRadius candidates from there
__global__ void __launch_bounds__(kThreads) ploc_nearest(const Box *__restrict__ boxes, uint32_t m, uint32_t *__restrict__ nn)
{
    constexpr uint32_t kSpan = kThreads + 2u * kPlocRadius;
    __shared__ float s[6][kSpan];
    const uint32_t base = blockIdx.x * kThreads;  // s[.][k] is cluster base - kPlocRadius + k
    for (uint32_t k = threadIdx.x; k < kSpan; k += kThreads) {
        const int64_t g = static_cast<int64_t>(base) - kPlocRadius + k;
        if (g >= 0 && g < static_cast<int64_t>(m)) {
            const Box b = boxes[g];
            for (int ax = 0; ax < 3; ++ax) s[ax][k] = b.lo[ax], s[3 + ax][k] = b.hi[ax];
        }
    }
    __syncthreads();
    const uint32_t i = base + threadIdx.x;
    if (i >= m) return;
    const uint32_t me = threadIdx.x + kPlocRadius;
    const float lo[3] = {s[0][me], s[1][me], s[2][me]}, hi[3] = {s[3][me], s[4][me], s[5][me]};
    const uint32_t first = i > kPlocRadius ? i - kPlocRadius : 0u, last = min(m - 1u, i + kPlocRadius);
    double best_d = 0.0;
    uint32_t best_j = kNone;
    for (uint32_t j = first; j <= last; ++j) {
        if (j == i) continue;
        const uint32_t k = j - base + kPlocRadius;  // (j + kPlocRadius >= base: j >= i - kPlocRadius >= base - kPlocRadius)
        const float blo[3] = {s[0][k], s[1][k], s[2][k]}, bhi[3] = {s[3][k], s[4][k], s[5][k]};
        const double d = union_half_area(lo, hi, blo, bhi);
        if (better(d, i, j, best_d, best_j)) best_d = d, best_j = j;
    }
    nn[i] = best_j;  // (m >= 2: every cluster has a candidate)
}

// keep[i] = 0 for the right member of a mutual pair; the scan runs over one word more
__global__ void ploc_keep(const uint32_t *__restrict__ nn, uint32_t m, uint32_t *__restrict__ keep)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    uint32_t k = 0u;
    if (i < m) {
        const uint32_t j = nn[i];
        k = (j < m && j < i && nn[j] == i) ? 0u : 1u;
    }
    keep[i] = k;
}

// behind the scan of keep: a kept cluster moves to position pos[i]; the left member of a mutual pair (i, j) becomes the inner node n + (n - m) + (number of
// clusters removed before j) — a provisional name, unique because every merge removes one cluster — and writes its child pair
__global__ void ploc_merge(const Box *__restrict__ boxes, const uint32_t *__restrict__ ids, const uint32_t *__restrict__ nn, const uint32_t *__restrict__ keep,
                           const uint32_t *__restrict__ pos, uint32_t m, uint32_t n, Box *__restrict__ boxes_out, uint32_t *__restrict__ ids_out, uint2 *__restrict__ children)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || !keep[i]) return;
    const uint32_t p = pos[i];
    if (p >= m) return;
    Box b = boxes[i];
    uint32_t id = ids[i];
    const uint32_t j = nn[i];
    if (j < m && j > i && nn[j] == i) {
        const uint32_t inner = (n - m) + (j - pos[j]);
        if (inner >= n - 1u) return;  // (n - 1 inner nodes in all: a stray word must not become an address)
        const Box r = boxes[j];
        for (int ax = 0; ax < 3; ++ax) b.lo[ax] = fminf(b.lo[ax], r.lo[ax]), b.hi[ax] = fmaxf(b.hi[ax], r.hi[ax]);
        children[inner] = make_uint2(id, ids[j]);
        id = n + inner;
    }
    boxes_out[p] = b;
    ids_out[p] = id;
}

// The tail: the last m <= kPlocTailClusters clusters finished by one work-group, one lane per cluster, the same iteration in LDS until one cluster is left or
// the iterations run out.  counters[kPlocRoot] = the provisional node of the root, counters[kPlocIterations] = iterations in all (0xFFFFFFFF: ran out).
__global__ void __launch_bounds__(kPlocTailClusters) ploc_tail(const Box *__restrict__ boxes, const uint32_t *__restrict__ ids, uint32_t m, uint32_t n, uint32_t iterations,
                                                               uint2 *__restrict__ children, uint32_t *__restrict__ counters)
{
    __shared__ float s[6][kPlocTailClusters];
    __shared__ uint32_t s_id[kPlocTailClusters], s_nn[kPlocTailClusters], s_scan[kPlocTailClusters];
    const uint32_t t = threadIdx.x;
    if (blockIdx.x != 0 || m > kPlocTailClusters) return;
    if (t < m) {
        const Box b = boxes[t];
        for (int ax = 0; ax < 3; ++ax) s[ax][t] = b.lo[ax], s[3 + ax][t] = b.hi[ax];
        s_id[t] = ids[t];
    }
    __syncthreads();
    while (m > 1u && iterations < kPlocMaxIterations) {  // (m and iterations are uniform over the work-group)
        float lo[3], hi[3];
        if (t < m) {
            for (int ax = 0; ax < 3; ++ax) lo[ax] = s[ax][t], hi[ax] = s[3 + ax][t];
            const uint32_t first = t > kPlocRadius ? t - kPlocRadius : 0u, last = min(m - 1u, t + kPlocRadius);
            double best_d = 0.0;
            uint32_t best_j = kNone;
            for (uint32_t j = first; j <= last; ++j) {
                if (j == t) continue;
                const float blo[3] = {s[0][j], s[1][j], s[2][j]}, bhi[3] = {s[3][j], s[4][j], s[5][j]};
                const double d = union_half_area(lo, hi, blo, bhi);
                if (better(d, t, j, best_d, best_j)) best_d = d, best_j = j;
            }
            s_nn[t] = best_j;
        }
        __syncthreads();
        uint32_t partner = kNone, keep = 0u;
        if (t < m) {
            const uint32_t j = s_nn[t];
            if (j < m && s_nn[j] == t) partner = j;
            keep = (partner != kNone && partner < t) ? 0u : 1u;
        }
        s_scan[t] = keep;
        __syncthreads();
        for (uint32_t off = 1u; off < kPlocTailClusters; off <<= 1) {  // an inclusive scan of the keep flags
            const uint32_t v = t >= off ? s_scan[t - off] : 0u;
            __syncthreads();
            s_scan[t] += v;
            __syncthreads();
        }
        const uint32_t kept = s_scan[kPlocTailClusters - 1u];
        uint32_t id = 0u;
        if (t < m && keep) {
            id = s_id[t];
            if (partner != kNone) {
                const uint32_t inner = (n - m) + (partner - s_scan[partner]);  // partner is removed: its inclusive and exclusive sums are equal
                for (int ax = 0; ax < 3; ++ax) lo[ax] = fminf(lo[ax], s[ax][partner]), hi[ax] = fmaxf(hi[ax], s[3 + ax][partner]);
                if (inner < n - 1u) children[inner] = make_uint2(id, s_id[partner]);
                id = n + inner;
            }
        }
        const uint32_t p = s_scan[t] - keep;
        __syncthreads();
        if (t < m && keep) {
            for (int ax = 0; ax < 3; ++ax) s[ax][p] = lo[ax], s[3 + ax][p] = hi[ax];
            s_id[p] = id;
        }
        m = kept;
        iterations += 1u;
        __syncthreads();
    }
    if (t == 0u) {
        counters[kPlocRoot] = s_id[0];
        counters[kPlocIterations] = m > 1u ? kNone : iterations;
    }
}

__global__ void layout_root(const uint32_t *__restrict__ counters, uint32_t n, uint32_t *__restrict__ cur, uint32_t *__restrict__ flags, float4 *__restrict__ nodes)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t root = counters[kPlocRoot];
    cur[0] = root;
    flags[0] = root >= n ? 1u : 0u;
    flags[1] = 0u;
    nodes[2] = nodes[3] = make_float4(0.f, 0.f, 0.f, 0.f);  // slot 1 of the layout is unused
}

// One level of the layout, behind the scan of its flags (the shape of rvpt_build.hip: emit_level): node j of the level is the provisional node cur[j]; a leaf
// becomes (its sorted position, 1), an inner node gets the pair next_begin + 2 offs[j] and hands its two children to the next level.
__global__ void layout_level(const uint2 *__restrict__ children, const uint32_t *__restrict__ cur, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ offs, uint32_t n,
                             uint32_t begin, uint32_t count, uint32_t next_begin, uint32_t *__restrict__ cur_next, uint32_t *__restrict__ flags_next, float4 *__restrict__ nodes,
                             uint32_t node_cap)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count || begin + j >= node_cap) return;
    const uint32_t id = cur[j], off = offs[j];
    uint32_t first = id, cnt = 1u;
    if (flags[j]) {
        const uint32_t inner = id - n;
        if (inner >= n - 1u || 2u * off + 1u >= n) return;  // (a level has at most n nodes; the host fails a build whose levels do not add up)
        const uint2 c = children[inner];
        first = next_begin + 2u * off, cnt = 0u;
        cur_next[2u * off] = c.x, cur_next[2u * off + 1u] = c.y;
        flags_next[2u * off] = c.x >= n ? 1u : 0u;
        flags_next[2u * off + 1u] = c.y >= n ? 1u : 0u;
    } else if (id >= n) {
        return;
    }
    if (j == count - 1u) flags_next[2u * (off + flags[j])] = 0u;  // the next level's scan runs over one word more than it has nodes
    nodes[2u * (begin + j)] = make_float4(__uint_as_float(first), __uint_as_float(cnt), 0.f, 0.f);
    nodes[2u * (begin + j) + 1u] = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace

// scratch, in bytes per region: the child pairs of the n - 1 provisional inner nodes (8 n), the cluster boxes twice (2 x 24 n), the clusters' provisional nodes
// twice (2 x 4 n), the nearest neighbours (4 n)
size_t ploc_scratch_bytes(uint32_t n) { return 68u * static_cast<size_t>(n); }

namespace {
struct Regions {
    Box *boxes, *boxes_out;
    uint32_t *ids, *ids_out, *nn;
    uint2 *children;
};
Regions regions(unsigned char *scratch, uint32_t n, uint32_t parity)
{
    const size_t N = n;
    Box *const b = reinterpret_cast<Box *>(scratch + 8u * N);
    uint32_t *const w = reinterpret_cast<uint32_t *>(scratch + 56u * N);
    return Regions{b + (parity ? N : 0u), b + (parity ? 0u : N), w + (parity ? N : 0u), w + (parity ? 0u : N), w + 2u * N, reinterpret_cast<uint2 *>(scratch)};
}
}  // namespace

hipError_t ploc_begin(hipStream_t stream, const float4 *tris, uint32_t n, unsigned char *scratch)
{
    const Regions r = regions(scratch, n, 0u);
    hipLaunchKernelGGL(ploc_init, dim3(blocks_for(n)), dim3(kThreads), 0, stream, tris, n, r.boxes, r.ids);
    return hipGetLastError();
}

hipError_t ploc_iteration(hipStream_t stream, void *temp, size_t temp_bytes, unsigned char *scratch, uint32_t n, uint32_t m, uint32_t parity, uint32_t *keep, uint32_t *pos)
{
    const Regions r = regions(scratch, n, parity);
    hipLaunchKernelGGL(ploc_nearest, dim3(blocks_for(m)), dim3(kThreads), 0, stream, r.boxes, m, r.nn);
    hipLaunchKernelGGL(ploc_keep, dim3(blocks_for(m + 1u)), dim3(kThreads), 0, stream, r.nn, m, keep);
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, keep, pos, 0u, static_cast<size_t>(m) + 1u, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ploc_merge, dim3(blocks_for(m)), dim3(kThreads), 0, stream, r.boxes, r.ids, r.nn, keep, pos, m, n, r.boxes_out, r.ids_out, r.children);
    return hipGetLastError();
}

hipError_t ploc_finish(hipStream_t stream, unsigned char *scratch, uint32_t n, uint32_t m, uint32_t parity, uint32_t iterations, uint32_t *counters)
{
    const Regions r = regions(scratch, n, parity);
    hipLaunchKernelGGL(ploc_tail, dim3(1), dim3(kPlocTailClusters), 0, stream, r.boxes, r.ids, m, n, iterations, r.children, counters);
    return hipGetLastError();
}

hipError_t ploc_layout_root(hipStream_t stream, const uint32_t *counters, uint32_t n, uint32_t *cur, uint32_t *flags, float4 *nodes)
{
    hipLaunchKernelGGL(layout_root, dim3(1), dim3(64), 0, stream, counters, n, cur, flags, nodes);
    return hipGetLastError();
}

hipError_t ploc_layout_level(hipStream_t stream, void *temp, size_t temp_bytes, const unsigned char *scratch, uint32_t n, const uint32_t *cur, const uint32_t *flags, uint32_t *offs,
                             uint32_t begin, uint32_t count, uint32_t next_begin, uint32_t *cur_next, uint32_t *flags_next, float4 *nodes, uint32_t node_cap)
{
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, flags, offs, 0u, static_cast<size_t>(count) + 1u, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(layout_level, dim3(blocks_for(count)), dim3(kThreads), 0, stream, reinterpret_cast<const uint2 *>(scratch), cur, flags, offs, n, begin,
                       count, next_begin, cur_next, flags_next, nodes, node_cap);
    return hipGetLastError();
}

}  // namespace rv
