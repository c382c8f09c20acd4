// rvpt_build.hip — the device BVH build's kernels (rvpt_build.h holds the specification of the tree): keys, rocPRIM's radix sort, the gather into leaf order,
// the topology level by level in the breadth-first device layout, and the 4-wide form as the same kind of level loop.  Not frame kernels: this file is outside
// build.py's KERNEL_SOURCES, so the frame kernels' identity (kernel_sha) and the profiles stamped with it stand.
//
// The target is latency, not bandwidth: a level is a scan and one kernel, and the host reads one word per level.  Every kernel is one thread per item with its
// bounds checked against the capacity of what it writes; no kernel waits on another work-group, counters are written with ordinary atomics on vector memory.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "rvpt_build.h"

namespace rv {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // == kWideEmpty / kWideFormEmpty

inline uint32_t blocks_for(uint32_t n) { return (n + kThreads - 1u) / kThreads; }

// floats as integers of the same order (for atomicMin / atomicMax): -0 sorts below +0, which no later step can tell apart
__device__ inline uint32_t ordered(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float unordered(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }

__device__ inline float centroid(float a, float b, float c) { return (a + b + c) * (1.0f / 3.0f); }

__global__ void reset_counters(uint32_t *__restrict__ counters)
{
    const uint32_t t = threadIdx.x;
    if (t >= kBuildCounters) return;
    // first bad = none, max leaf = 0, lo = the largest ordered value, hi = the smallest
    counters[t] = (t == kBuildFirstBad || (t >= kBuildBounds && t < kBuildBounds + 3u)) ? 0xFFFFFFFFu : 0u;
}

// materials[int(mat_id.x)] must stay inside the buffer: the test of the host loop in rvpt_hip_upload_scene, the smallest offending index kept
__global__ void validate_materials(const float4 *__restrict__ src, uint32_t n_tris, uint32_t n_mats, uint32_t *__restrict__ counters)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris) return;
    const float m = src[4u * i + 3u].x;
    const bool ok = m >= 0.0f && m < 2147483648.0f && static_cast<uint32_t>(static_cast<int>(m)) < n_mats;
    if (!ok) atomicMin(&counters[kBuildFirstBad], i);
}

__global__ void centroid_bounds(const float4 *__restrict__ src, uint32_t n_tris, uint32_t *__restrict__ counters)
{
    __shared__ uint32_t s[6];
    if (threadIdx.x < 6u) s[threadIdx.x] = threadIdx.x < 3u ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_tris; i += gridDim.x * blockDim.x) {
        const float4 a = src[4u * i], b = src[4u * i + 1u], c = src[4u * i + 2u];
        const float cen[3] = {centroid(a.x, b.x, c.x), centroid(a.y, b.y, c.y), centroid(a.z, b.z, c.z)};
        for (int ax = 0; ax < 3; ++ax)
            if (cen[ax] == cen[ax]) {  // a NaN takes no part
                const uint32_t e = ordered(cen[ax]);
                lo[ax] = min(lo[ax], e), hi[ax] = max(hi[ax], e);
            }
    }
    for (int ax = 0; ax < 3; ++ax) {
        atomicMin(&s[ax], lo[ax]);
        atomicMax(&s[3 + ax], hi[ax]);
    }
    __syncthreads();
    if (threadIdx.x < 3u) atomicMin(&counters[kBuildBounds + threadIdx.x], s[threadIdx.x]);
    else if (threadIdx.x < 6u) atomicMax(&counters[kBuildBounds + threadIdx.x], s[threadIdx.x]);
}

__device__ inline uint32_t quantise(float c, float lo, float hi)
{
    const float ext = hi - lo;
    if (!(ext > 0.0f)) return 0u;
    const float f = (c - lo) * (1024.0f / ext);
    return f >= 1023.0f ? 1023u : (f >= 0.0f ? static_cast<uint32_t>(static_cast<int>(f)) : 0u);
}

// 10 bits -> every third bit
__device__ inline uint32_t spread3(uint32_t x)
{
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__global__ void make_keys(const float4 *__restrict__ src, uint32_t n_tris, const uint32_t *__restrict__ counters, uint64_t *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris) return;
    const float4 a = src[4u * i], b = src[4u * i + 1u], c = src[4u * i + 2u];
    const uint32_t qx = quantise(centroid(a.x, b.x, c.x), unordered(counters[kBuildBounds + 0]), unordered(counters[kBuildBounds + 3]));
    const uint32_t qy = quantise(centroid(a.y, b.y, c.y), unordered(counters[kBuildBounds + 1]), unordered(counters[kBuildBounds + 4]));
    const uint32_t qz = quantise(centroid(a.z, b.z, c.z), unordered(counters[kBuildBounds + 2]), unordered(counters[kBuildBounds + 5]));
    const uint32_t code = (spread3(qx) << 2) | (spread3(qy) << 1) | spread3(qz);
    keys[i] = (static_cast<uint64_t>(code) << 32) | i;
}

// one thread per quad: 64 consecutive bytes of a record by four neighbouring lanes
__global__ void gather_records(const float4 *__restrict__ src, const uint64_t *__restrict__ sorted_keys, uint32_t n_tris, float4 *__restrict__ out, uint32_t *__restrict__ perm)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t >> 2, q = t & 3u;
    if (j >= n_tris) return;
    const uint32_t i = static_cast<uint32_t>(sorted_keys[j]);
    if (i >= n_tris) return;  // (a key's low word is a caller's index; a stray word must not become an address)
    out[4u * j + q] = src[4u * i + q];
    if (q == 0u) perm[j] = i;
}

__global__ void gather_vertex_rows(const float4 *__restrict__ src, const uint32_t *__restrict__ perm, uint32_t n_tris, float4 *__restrict__ tris)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t >> 2, q = t & 3u;
    if (j >= n_tris || q == 3u) return;  // the mat_id row stays
    const uint32_t i = perm[j];
    if (i >= n_tris) return;
    tris[4u * j + q] = src[4u * i + q];
}

__global__ void root_level(uint32_t n_tris, uint2 *__restrict__ ranges, uint32_t *__restrict__ flags, float4 *__restrict__ nodes)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    ranges[0] = make_uint2(0u, n_tris - 1u);
    flags[0] = n_tris > kLbvhLeafTris ? 1u : 0u;
    flags[1] = 0u;
    nodes[2] = nodes[3] = make_float4(0.f, 0.f, 0.f, 0.f);  // slot 1 of the layout is unused
}

// One level of the topology, behind the scan of its flags: node j of the level (device index begin + j) becomes a leaf or an inner node whose children are the
// pair next_begin + 2 offs[j]; the children's ranges and flags are the next level's.  Only the two head words of a node mean anything until refit_level runs.
__global__ void emit_level(const uint64_t *__restrict__ keys, const uint2 *__restrict__ ranges, const uint32_t *__restrict__ flags, const uint32_t *__restrict__ offs,
                           uint32_t begin, uint32_t count, uint32_t next_begin, uint2 *__restrict__ ranges_next, uint32_t *__restrict__ flags_next,
                           float4 *__restrict__ nodes, uint32_t node_cap, uint32_t *__restrict__ counters)
{
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < count && begin + j < node_cap) {
        const uint2 r = ranges[j];
        const uint32_t a = r.x, b = r.y, off = offs[j];
        uint32_t first, cnt;
        if (!flags[j]) {
            first = a, cnt = b - a + 1u;
            atomicMax(&s_max, cnt);
        } else {
            const uint64_t ka = keys[a];
            const uint32_t p = 63u - static_cast<uint32_t>(__clzll(static_cast<long long>(ka ^ keys[b])));
            uint32_t lo = a, hi = b;  // bit p of key[lo] is 0, of key[hi] 1
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if ((keys[mid] >> p) & 1ull) hi = mid;
                else lo = mid;
            }
            first = next_begin + 2u * off, cnt = 0u;
            ranges_next[2u * off] = make_uint2(a, hi - 1u);
            ranges_next[2u * off + 1u] = make_uint2(hi, b);
            flags_next[2u * off] = (hi - a) > kLbvhLeafTris ? 1u : 0u;
            flags_next[2u * off + 1u] = (b - hi + 1u) > kLbvhLeafTris ? 1u : 0u;
        }
        if (j == count - 1u) flags_next[2u * (off + flags[j])] = 0u;  // the next level's scan runs over one word more than it has nodes
        nodes[2u * (begin + j)] = make_float4(__uint_as_float(first), __uint_as_float(cnt), 0.f, 0.f);
        nodes[2u * (begin + j) + 1u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(&counters[kBuildMaxLeaf], s_max);
}

struct Node {
    uint32_t first, count;
    float b[6];  // minx maxx miny maxy minz maxz
};
__device__ inline Node load_node(const float4 *__restrict__ nodes, uint32_t i)
{
    const float4 q0 = nodes[2u * i], q1 = nodes[2u * i + 1u];
    return Node{__float_as_uint(q0.x), __float_as_uint(q0.y), {q0.z, q0.w, q1.x, q1.y, q1.z, q1.w}};
}
__device__ inline bool contains(const Node &a, const Node &b)
{
    for (int ax = 0; ax < 3; ++ax)
        if (!(b.b[2 * ax] >= a.b[2 * ax] && b.b[2 * ax + 1] <= a.b[2 * ax + 1])) return false;
    return true;
}
__device__ inline double area(const Node &n)  // bvh_wide.cpp: area, the same operations in the same order (no contraction: -ffp-contract=off)
{
    const double dx = double(n.b[1]) - n.b[0], dy = double(n.b[3]) - n.b[2], dz = double(n.b[5]) - n.b[4];
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dy), __dmul_rn(dy, dz)), __dmul_rn(dz, dx));
}

__global__ void wide_root(uint32_t *__restrict__ bin)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) bin[0] = 0u;
}

// bvh_wide.cpp: regroup for one wide node: [left, right], the inner child of largest area (first maximum) replaced in place by its two children until four.
// Writes the node's d_wide_map row, its leaf heads (inner slots: filled by wide_emit) and how many inner children it has.
__global__ void wide_pick(const float4 *__restrict__ nodes, uint32_t n_nodes, const uint32_t *__restrict__ bin, uint32_t wbase, uint32_t count, uint32_t head_shift,
                          uint32_t *__restrict__ cnt, uint32_t *__restrict__ wide_map, uint32_t *__restrict__ heads, uint32_t wide_cap)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > count) return;
    if (j == count) {  // the scan runs over one word more
        cnt[j] = 0u;
        return;
    }
    cnt[j] = 0u;
    const uint32_t w = wbase + j, root = bin[j];
    // (a guard, not a result: a level that does not fit wide_cap rows is left partly written, and the host, which reads the same count from offs[count],
    // fails the build before anything reads it — rvpt_scene.hip: build_scene_on_device)
    if (w >= wide_cap || root >= n_nodes) return;
    const uint32_t f0 = load_node(nodes, root).first;
    if (f0 >= n_nodes - 1u) return;
    uint32_t c[4] = {f0, f0 + 1u, kEmpty, kEmpty}, m = 2u;
    while (m < 4u) {
        int pick = -1;
        double best = -1.0;
        for (uint32_t i = 0; i < m; ++i) {
            const Node n = load_node(nodes, c[i]);
            if (n.count > 0u || n.first >= n_nodes - 1u) continue;
            if (!contains(n, load_node(nodes, n.first)) || !contains(n, load_node(nodes, n.first + 1u))) continue;  // this box must be tested itself
            const double ar = area(n);
            if (ar > best) best = ar, pick = static_cast<int>(i);
        }
        if (pick < 0) break;
        const uint32_t f = load_node(nodes, c[pick]).first;
        for (uint32_t i = m; i > static_cast<uint32_t>(pick) + 1u; --i) c[i] = c[i - 1u];
        c[pick] = f, c[pick + 1] = f + 1u;
        m += 1u;
    }
    uint32_t inner = 0u;
    for (uint32_t i = 0; i < 4u; ++i) {
        uint32_t head = kEmpty;
        if (c[i] != kEmpty) {
            const Node n = load_node(nodes, c[i]);
            if (n.count > 0u) head = n.first | (n.count << head_shift);
            else inner += 1u;
        }
        wide_map[4u * w + i] = c[i];
        heads[4u * w + i] = head;
    }
    cnt[j] = inner;
}

// behind the scan of cnt: the inner children of wide node j of the level get the wide indices next_base + offs[j] .., in slot order (the host's queue order)
__global__ void wide_emit(const float4 *__restrict__ nodes, uint32_t n_nodes, uint32_t wbase, uint32_t count, const uint32_t *__restrict__ offs, const uint32_t *__restrict__ wide_map,
                          uint32_t *__restrict__ heads, uint32_t wide_cap, uint32_t *__restrict__ bin_next)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const uint32_t w = wbase + j;
    if (w >= wide_cap) return;
    uint32_t next = offs[j];
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t b = wide_map[4u * w + i];
        if (b == kEmpty || b >= n_nodes || __float_as_uint(nodes[2u * b].y) > 0u) continue;
        if (wbase + count + next >= wide_cap) return;  // (as in wide_pick: the host's check of offs[count] fails such a build)
        heads[4u * w + i] = wbase + count + next;
        bin_next[next] = b;
        next += 1u;
    }
}

__global__ void wide_heads(const uint32_t *__restrict__ heads, uint32_t n_wide, float *__restrict__ wide)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4u * n_wide) return;
    wide[static_cast<size_t>(t >> 2) * 32u + 24u + (t & 3u)] = __uint_as_float(heads[t]);
}

__global__ void wide_need(const float *__restrict__ wide, uint32_t wbase, uint32_t count, uint32_t n_wide, uint32_t head_shift, uint32_t *__restrict__ need)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count || wbase + j >= n_wide) return;
    const uint32_t w = wbase + j;
    uint32_t head[4], n_children = 0u;
    for (uint32_t i = 0; i < 4u; ++i) {
        head[i] = __float_as_uint(wide[static_cast<size_t>(w) * 32u + 24u + i]);
        n_children += head[i] != kEmpty;
    }
    uint32_t worst = 0u;
    for (uint32_t i = 0; i < n_children; ++i) {
        const bool leaf = (head[i] >> head_shift) != 0u;
        const uint32_t below = (leaf || head[i] >= n_wide) ? 0u : need[head[i]];  // an inner child lies on a deeper level: written by an earlier launch
        worst = max(worst, (n_children - 1u - i) + below);
    }
    need[w] = worst;
}

}  // namespace

hipError_t build_validate_materials(hipStream_t stream, const float4 *src, uint32_t n_tris, uint32_t n_mats, uint32_t *counters)
{
    hipLaunchKernelGGL(reset_counters, dim3(1), dim3(64), 0, stream, counters);
    hipLaunchKernelGGL(validate_materials, dim3(blocks_for(n_tris)), dim3(kThreads), 0, stream, src, n_tris, n_mats, counters);
    return hipGetLastError();
}

hipError_t build_keys(hipStream_t stream, const float4 *src, uint32_t n_tris, uint32_t *counters, uint64_t *keys)
{
    hipLaunchKernelGGL(reset_counters, dim3(1), dim3(64), 0, stream, counters);
    hipLaunchKernelGGL(centroid_bounds, dim3(std::min(blocks_for(n_tris), 1024u)), dim3(kThreads), 0, stream, src, n_tris, counters);
    hipLaunchKernelGGL(make_keys, dim3(blocks_for(n_tris)), dim3(kThreads), 0, stream, src, n_tris, counters, keys);
    return hipGetLastError();
}

hipError_t build_temp_bytes(uint32_t n_tris, size_t *bytes)
{
    size_t sort_bytes = 0, scan_bytes = 0;
    uint64_t *k = nullptr;
    uint32_t *u = nullptr;
    hipError_t e = rocprim::radix_sort_keys(nullptr, sort_bytes, k, k, n_tris, 0, 62, hipStream_t(nullptr));
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(nullptr, scan_bytes, u, u, 0u, static_cast<size_t>(n_tris) + 1u, rocprim::plus<uint32_t>(), hipStream_t(nullptr));
    if (e != hipSuccess) return e;
    *bytes = std::max(sort_bytes, scan_bytes);
    return hipSuccess;
}

hipError_t build_sort_keys(hipStream_t stream, void *temp, size_t temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, uint32_t n_tris)
{
    return rocprim::radix_sort_keys(temp, temp_bytes, keys_in, keys_out, n_tris, 0, 62, stream);  // 30 code bits above 32 index bits
}

hipError_t build_gather(hipStream_t stream, const float4 *src, const uint64_t *sorted_keys, uint32_t n_tris, float4 *tris_out, uint32_t *perm_out)
{
    const uint64_t threads = 4ull * n_tris;
    hipLaunchKernelGGL(gather_records, dim3(static_cast<uint32_t>((threads + kThreads - 1u) / kThreads)), dim3(kThreads), 0, stream, src, sorted_keys, n_tris, tris_out, perm_out);
    return hipGetLastError();
}

hipError_t build_gather_vertices(hipStream_t stream, const float4 *src, const uint32_t *perm, uint32_t n_tris, float4 *tris)
{
    const uint64_t threads = 4ull * n_tris;
    hipLaunchKernelGGL(gather_vertex_rows, dim3(static_cast<uint32_t>((threads + kThreads - 1u) / kThreads)), dim3(kThreads), 0, stream, src, perm, n_tris, tris);
    return hipGetLastError();
}

hipError_t build_root(hipStream_t stream, uint32_t n_tris, uint2 *ranges, uint32_t *flags, float4 *nodes)
{
    hipLaunchKernelGGL(root_level, dim3(1), dim3(64), 0, stream, n_tris, ranges, flags, nodes);
    return hipGetLastError();
}

hipError_t build_level(hipStream_t stream, void *temp, size_t temp_bytes, const uint64_t *sorted_keys, const uint2 *ranges, const uint32_t *flags, uint32_t *offs,
                       uint32_t begin, uint32_t count, uint32_t next_begin, uint2 *ranges_next, uint32_t *flags_next, float4 *nodes, uint32_t node_cap, uint32_t *counters)
{
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, flags, offs, 0u, static_cast<size_t>(count) + 1u, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(emit_level, dim3(blocks_for(count)), dim3(kThreads), 0, stream, sorted_keys, ranges, flags, offs, begin, count, next_begin, ranges_next, flags_next, nodes,
                       node_cap, counters);
    return hipGetLastError();
}

hipError_t build_wide_root(hipStream_t stream, uint32_t *bin)
{
    hipLaunchKernelGGL(wide_root, dim3(1), dim3(64), 0, stream, bin);
    return hipGetLastError();
}

hipError_t build_wide_level(hipStream_t stream, void *temp, size_t temp_bytes, const float4 *nodes, uint32_t n_nodes, const uint32_t *bin, uint32_t wbase, uint32_t count,
                            uint32_t head_shift, uint32_t *cnt, uint32_t *offs, uint32_t *wide_map, uint32_t *heads, uint32_t wide_cap, uint32_t *bin_next)
{
    hipLaunchKernelGGL(wide_pick, dim3(blocks_for(count + 1u)), dim3(kThreads), 0, stream, nodes, n_nodes, bin, wbase, count, head_shift, cnt, wide_map, heads, wide_cap);
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, cnt, offs, 0u, static_cast<size_t>(count) + 1u, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wide_emit, dim3(blocks_for(count)), dim3(kThreads), 0, stream, nodes, n_nodes, wbase, count, offs, wide_map, heads, wide_cap, bin_next);
    return hipGetLastError();
}

hipError_t build_wide_heads(hipStream_t stream, const uint32_t *heads, uint32_t n_wide, float *wide)
{
    hipLaunchKernelGGL(wide_heads, dim3(blocks_for(4u * n_wide)), dim3(kThreads), 0, stream, heads, n_wide, wide);
    return hipGetLastError();
}

hipError_t build_wide_need(hipStream_t stream, const float *wide, uint32_t wbase, uint32_t count, uint32_t n_wide, uint32_t head_shift, uint32_t *need)
{
    hipLaunchKernelGGL(wide_need, dim3(blocks_for(count)), dim3(kThreads), 0, stream, wide, wbase, count, n_wide, head_shift, need);
    return hipGetLastError();
}

}  // namespace rv
