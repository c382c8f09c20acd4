// rvpt_sah.hip — the SAH build form's kernels (rvpt_build.h: THE SAH TREE holds the specification): rvpt_bvh_build's top-down binned-SAH build run level by
// level on the device, every unstable step made stable, the tree written straight into the breadth-first device layout.  Not frame kernels: this file is outside
// build.py's KERNEL_SOURCES, so the frame kernels' identity (kernel_sha) and the profiles stamped with it stand.
//
// A level is: (a) bounds, centroid bounds and 3 x 16 bins per node — nodes of more than kSahLargeNode triangles are shared by work-groups that each cover
// kSahChunk positions of the index array, pre-reduce in LDS and merge through atomic min / max on order-preserving integers and integer adds (exact, whatever
// the order), every other node is reduced by one wave whose bins never leave LDS; (b) the decision by that wave; (d) the scan of the "splits" flags and the
// emit; the host reads three words; (c) the partition into the other half of the double-buffered index array.  Every kernel checks what it indexes against the
// capacity of what it writes; no kernel waits on another work-group.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cfloat>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "rvpt_build.h"

namespace rv {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kWavesPerGroup = 4;
// one node's reduction: bounds lo xyz, hi xyz, centroid bounds lo xyz, hi xyz, then per (axis, bin) a box (lo xyz, hi xyz) and a count, all as ordered integers
constexpr uint32_t kBinWords = 7, kNodeWords = 12u + 3u * kSahBins * kBinWords;
constexpr uint32_t kKindLeaf = 0, kKindBinned = 1, kKindMedian = 2;

inline uint32_t blocks_for(uint32_t n) { return (n + kThreads - 1u) / kThreads; }

// floats as integers of the same order (rvpt_build.hip: ordered); a NaN never gets here, so 0xFFFFFFFF and 0 are free to mean "nothing yet"
__device__ inline uint32_t ordered(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float unordered(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }
// the host's Box: it starts at +-FLT_MAX and takes std::min / std::max, so a side on which nothing took part, or nothing but +inf (-inf for a high side), is
// +-FLT_MAX — never an infinity of that sign (lo = hi = +inf would make the extent a NaN where the host's is +inf, and another median axis: tests/test_device_state.py)
__device__ inline float lo_of(uint32_t e) { return e == 0xFFFFFFFFu ? FLT_MAX : fminf(unordered(e), FLT_MAX); }
__device__ inline float hi_of(uint32_t e) { return e == 0u ? -FLT_MAX : fmaxf(unordered(e), -FLT_MAX); }
__device__ inline uint32_t initial_word(uint32_t w) { return (w < 12u ? (w % 6u) < 3u : ((w - 12u) % kBinWords) < 3u) ? 0xFFFFFFFFu : 0u; }

__device__ inline int bin_of(float c, float lo, float scale)
{
    const float f = (c - lo) * scale;
    return f >= static_cast<float>(kSahBins - 1u) ? static_cast<int>(kSahBins - 1u) : (f >= 0.0f ? static_cast<int>(f) : 0);
}

__device__ inline float half_area(const float lo[3], const float hi[3])
{
    float d[3];
    for (int a = 0; a < 3; ++a) {
        const float e = hi[a] - lo[a];
        d[a] = e < 0.0f ? 0.0f : e;
    }
    return d[0] * (d[1] + d[2]) + d[1] * d[2];
}

struct Scratch {
    float *tri;  // SoA over the caller's index: 0..2 box lo, 3..5 box hi, 6..8 centroid
    uint32_t *idx[2], *pnode[2], *pflag, *prank, *mflag, *mrank, *cpos, *key32[2];
    uint64_t *key64[2];
    uint2 *ranges[2];
    uint32_t *nslot[2], *nflags, *offs, *dec, *nleft, *lbins;
    float *dlo, *dscale;
    uint32_t large_cap;
};

inline size_t words_of(uint32_t n) { return ((static_cast<size_t>(n) + 1u) * 4u + 15u) & ~size_t(15); }
inline uint32_t large_cap_of(uint32_t n) { return n / kSahLargeNode + 2u; }

Scratch carve(unsigned char *base, uint32_t n, size_t *total = nullptr)
{
    Scratch s;
    const size_t N = n, W = words_of(n);
    unsigned char *p = base;
    auto take = [&](size_t bytes) {
        unsigned char *q = p;
        p += (bytes + 15u) & ~size_t(15);
        return q;
    };
    for (int i = 0; i < 2; ++i) s.key64[i] = reinterpret_cast<uint64_t *>(take(8u * N));
    for (int i = 0; i < 2; ++i) s.ranges[i] = reinterpret_cast<uint2 *>(take(8u * (N + 1u)));
    s.tri = reinterpret_cast<float *>(take(36u * N));
    for (int i = 0; i < 2; ++i) s.idx[i] = reinterpret_cast<uint32_t *>(take(W));
    for (int i = 0; i < 2; ++i) s.pnode[i] = reinterpret_cast<uint32_t *>(take(W));
    s.pflag = reinterpret_cast<uint32_t *>(take(W)), s.prank = reinterpret_cast<uint32_t *>(take(W));
    s.mflag = reinterpret_cast<uint32_t *>(take(W)), s.mrank = reinterpret_cast<uint32_t *>(take(W));
    s.cpos = reinterpret_cast<uint32_t *>(take(W));
    for (int i = 0; i < 2; ++i) s.key32[i] = reinterpret_cast<uint32_t *>(take(W));
    for (int i = 0; i < 2; ++i) s.nslot[i] = reinterpret_cast<uint32_t *>(take(W));
    s.nflags = reinterpret_cast<uint32_t *>(take(W)), s.offs = reinterpret_cast<uint32_t *>(take(W));
    s.dec = reinterpret_cast<uint32_t *>(take(W)), s.nleft = reinterpret_cast<uint32_t *>(take(W));
    s.dlo = reinterpret_cast<float *>(take(W)), s.dscale = reinterpret_cast<float *>(take(W));
    s.large_cap = large_cap_of(n);
    s.lbins = reinterpret_cast<uint32_t *>(take(static_cast<size_t>(s.large_cap) * kNodeWords * 4u));
    if (total) *total = static_cast<size_t>(p - base);
    return s;
}

// per triangle of the caller's order: box, centroid, the iota; the root level
__global__ void sah_init(const float4 *__restrict__ src, uint32_t n, float *__restrict__ tri, uint32_t *__restrict__ idx, uint32_t *__restrict__ pnode, uint2 *__restrict__ ranges,
                         uint32_t *__restrict__ nslot, uint32_t *__restrict__ counters, float4 *__restrict__ nodes)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0u) {
        ranges[0] = make_uint2(0u, n);
        nslot[0] = n > kSahLargeNode ? 0u : kNone;
        counters[kBuildMaxLeaf] = 0u;
        counters[kSahSplits] = counters[kSahMedianTris] = counters[kSahLargeNext] = 0u;
        nodes[2] = nodes[3] = make_float4(0.f, 0.f, 0.f, 0.f);  // slot 1 of the layout is unused
    }
    if (i >= n) return;
    const float4 a = src[4u * i], b = src[4u * i + 1u], c = src[4u * i + 2u];
    const size_t N = n;
    tri[0u * N + i] = fminf(fminf(a.x, b.x), c.x), tri[3u * N + i] = fmaxf(fmaxf(a.x, b.x), c.x);
    tri[1u * N + i] = fminf(fminf(a.y, b.y), c.y), tri[4u * N + i] = fmaxf(fmaxf(a.y, b.y), c.y);
    tri[2u * N + i] = fminf(fminf(a.z, b.z), c.z), tri[5u * N + i] = fmaxf(fmaxf(a.z, b.z), c.z);
    tri[6u * N + i] = (a.x + b.x + c.x) * (1.0f / 3.0f);
    tri[7u * N + i] = (a.y + b.y + c.y) * (1.0f / 3.0f);
    tri[8u * N + i] = (a.z + b.z + c.z) * (1.0f / 3.0f);
    idx[i] = i;
    pnode[i] = 0u;
}

__global__ void sah_large_reset(uint32_t *__restrict__ lbins, uint32_t n_large)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_large * kNodeWords) return;
    lbins[t] = initial_word(t % kNodeWords);
}

// grows words 0..11 of a node's reduction by triangle ti (a NaN takes no part)
__device__ inline void grow_bounds(uint32_t *w, const float *__restrict__ tri, size_t N, uint32_t ti)
{
    for (uint32_t a = 0; a < 3u; ++a) {
        const float lo = tri[a * N + ti], hi = tri[(3u + a) * N + ti], c = tri[(6u + a) * N + ti];
        if (lo == lo) atomicMin(&w[a], ordered(lo));
        if (hi == hi) atomicMax(&w[3u + a], ordered(hi));
        if (c == c) atomicMin(&w[6u + a], ordered(c)), atomicMax(&w[9u + a], ordered(c));
    }
}

// grows the bins of a node's reduction by triangle ti; clo / scale: per axis, scale 0 = the axis has no extent
__device__ inline void grow_bins(uint32_t *w, const float *__restrict__ tri, size_t N, uint32_t ti, const float clo[3], const float scale[3], const bool live[3])
{
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!live[a]) continue;
        const int b = bin_of(tri[(6u + a) * N + ti], clo[a], scale[a]);
        uint32_t *bin = w + 12u + (a * kSahBins + static_cast<uint32_t>(b)) * kBinWords;
        for (uint32_t k = 0; k < 3u; ++k) {
            const float lo = tri[k * N + ti], hi = tri[(3u + k) * N + ti];
            if (lo == lo) atomicMin(&bin[k], ordered(lo));
            if (hi == hi) atomicMax(&bin[3u + k], ordered(hi));
        }
        atomicAdd(&bin[6], 1u);
    }
}

// The two large nodes a window of kSahChunk positions can meet: a node of more than kSahLargeNode >= kSahChunk triangles cannot lie strictly inside the window,
// so it holds the window's first or its last position.
struct Window {
    uint32_t first, end, node[2], slot[2];
};
__device__ inline Window window_of(const uint32_t *__restrict__ pnode, const uint32_t *__restrict__ nslot, uint32_t n, uint32_t m, uint32_t large_base, uint32_t n_large)
{
    Window w;
    w.first = blockIdx.x * kSahChunk;
    w.end = min(n, w.first + kSahChunk);
    w.node[0] = w.node[1] = w.slot[0] = w.slot[1] = kNone;
    if (w.first >= w.end) return w;
    const uint32_t j[2] = {pnode[w.first], pnode[w.end - 1u]};
    for (int k = 0; k < 2; ++k) {
        if (j[k] >= m || (k == 1 && j[1] == j[0])) continue;
        const uint32_t s = nslot[j[k]];
        if (s == kNone || s - large_base >= n_large) continue;
        w.node[k] = j[k], w.slot[k] = s - large_base;
    }
    return w;
}

// (a) for large nodes, first pass: bounds and centroid bounds
__global__ void __launch_bounds__(kThreads) sah_large_bounds(const float *__restrict__ tri, uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ pnode,
                                                             const uint32_t *__restrict__ nslot, uint32_t m, uint32_t large_base, uint32_t n_large, uint32_t *__restrict__ lbins)
{
    __shared__ uint32_t s[2][12];
    const Window w = window_of(pnode, nslot, n, m, large_base, n_large);
    if (w.slot[0] == kNone && w.slot[1] == kNone) return;  // (uniform over the work-group)
    if (threadIdx.x < 24u) s[threadIdx.x / 12u][threadIdx.x % 12u] = initial_word(threadIdx.x % 12u);
    __syncthreads();
    for (uint32_t p = w.first + threadIdx.x; p < w.end; p += kThreads) {
        const uint32_t j = pnode[p], ti = idx[p];
        const int k = (j == w.node[0]) ? 0 : (j == w.node[1] ? 1 : -1);
        if (k < 0 || j == kNone || ti >= n) continue;
        grow_bounds(s[k], tri, n, ti);
    }
    __syncthreads();
    if (threadIdx.x < 24u) {
        const uint32_t k = threadIdx.x / 12u, t = threadIdx.x % 12u;
        if (w.slot[k] != kNone) {
            uint32_t *dst = lbins + static_cast<size_t>(w.slot[k]) * kNodeWords + t;
            if ((t % 6u) < 3u) atomicMin(dst, s[k][t]);
            else atomicMax(dst, s[k][t]);
        }
    }
}

// (a) for large nodes, second pass: the bins over the centroid bounds the first pass left
__global__ void __launch_bounds__(kThreads) sah_large_bins(const float *__restrict__ tri, uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ pnode,
                                                           const uint32_t *__restrict__ nslot, uint32_t m, uint32_t large_base, uint32_t n_large, uint32_t *__restrict__ lbins)
{
    __shared__ uint32_t s[2][kNodeWords];
    const Window w = window_of(pnode, nslot, n, m, large_base, n_large);
    if (w.slot[0] == kNone && w.slot[1] == kNone) return;  // (uniform over the work-group)
    for (uint32_t t = threadIdx.x; t < 2u * kNodeWords; t += kThreads) s[t / kNodeWords][t % kNodeWords] = initial_word(t % kNodeWords);
    float clo[2][3], scale[2][3];
    bool live[2][3];
    for (int k = 0; k < 2; ++k)
        for (uint32_t a = 0; a < 3u; ++a) {
            clo[k][a] = scale[k][a] = 0.0f, live[k][a] = false;
            if (w.slot[k] == kNone) continue;
            const uint32_t *src = lbins + static_cast<size_t>(w.slot[k]) * kNodeWords;
            clo[k][a] = lo_of(src[6u + a]);
            const float extent = hi_of(src[9u + a]) - clo[k][a];
            live[k][a] = extent > 0.0f;
            scale[k][a] = static_cast<float>(kSahBins) / extent;
        }
    __syncthreads();
    for (uint32_t p = w.first + threadIdx.x; p < w.end; p += kThreads) {
        const uint32_t j = pnode[p], ti = idx[p];
        const int k = (j == w.node[0]) ? 0 : (j == w.node[1] ? 1 : -1);
        if (k < 0 || j == kNone || ti >= n) continue;
        grow_bins(s[k], tri, n, ti, clo[k], scale[k], live[k]);
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < 2u * (kNodeWords - 12u); t += kThreads) {
        const uint32_t k = t / (kNodeWords - 12u), word = 12u + t % (kNodeWords - 12u), r = (word - 12u) % kBinWords;
        if (w.slot[k] == kNone) continue;
        const uint32_t v = s[k][word];
        if (v == initial_word(word)) continue;  // an empty bin
        uint32_t *dst = lbins + static_cast<size_t>(w.slot[k]) * kNodeWords + word;
        if (r < 3u) atomicMin(dst, v);
        else if (r < 6u) atomicMax(dst, v);
        else atomicAdd(dst, v);
    }
}

// (a) for every other node and (b) for all: one wave per node of the level.  dec[j] = kind | axis << 2 | best_bin << 4.
__global__ void __launch_bounds__(kThreads) sah_decide(const float *__restrict__ tri, uint32_t n, const uint32_t *__restrict__ idx, const uint2 *__restrict__ ranges,
                                                       const uint32_t *__restrict__ nslot, const uint32_t *__restrict__ lbins, uint32_t large_base, uint32_t n_large, uint32_t m,
                                                       uint32_t depth, uint32_t *__restrict__ nflags, uint32_t *__restrict__ dec, float *__restrict__ dlo, float *__restrict__ dscale,
                                                       uint32_t *__restrict__ nleft, uint32_t *__restrict__ counters)
{
    __shared__ uint32_t s_all[kWavesPerGroup][kNodeWords];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t j = blockIdx.x * kWavesPerGroup + wave;
    uint32_t *s = s_all[wave];
    uint32_t begin = 0u, count = 0u, slot = kNone;
    if (j < m) {
        const uint2 r = ranges[j];
        begin = r.x, count = r.y;
        if (begin >= n || count > n - begin) count = 0u;  // (a stray range must not become an address)
        const uint32_t sl = nslot[j];
        if (sl != kNone && sl - large_base < n_large) slot = sl - large_base;
    }
    const bool active = count >= kSahMinLeaf;
    const bool binning = active && depth < kSahBalanceDepth;
    if (active) {
        for (uint32_t t = lane; t < kNodeWords; t += 64u) s[t] = slot != kNone ? lbins[static_cast<size_t>(slot) * kNodeWords + t] : initial_word(t);
    }
    __syncthreads();
    if (active && slot == kNone)
        for (uint32_t p = lane; p < count; p += 64u) {
            const uint32_t ti = idx[begin + p];
            if (ti < n) grow_bounds(s, tri, n, ti);
        }
    __syncthreads();
    float blo[3], bhi[3], clo[3], chi[3], scale[3];
    bool live[3];
    for (uint32_t a = 0; a < 3u; ++a) {
        blo[a] = bhi[a] = clo[a] = chi[a] = scale[a] = 0.0f, live[a] = false;
        if (!active) continue;
        blo[a] = lo_of(s[a]), bhi[a] = hi_of(s[3u + a]), clo[a] = lo_of(s[6u + a]), chi[a] = hi_of(s[9u + a]);
        const float extent = chi[a] - clo[a];
        live[a] = extent > 0.0f;
        scale[a] = static_cast<float>(kSahBins) / extent;
    }
    if (binning && slot == kNone)
        for (uint32_t p = lane; p < count; p += 64u) {
            const uint32_t ti = idx[begin + p];
            if (ti < n) grow_bins(s, tri, n, ti, clo, scale, live);
        }
    __syncthreads();
    // the two sweeps of one axis per lane (lanes 0..2), in the host code's order
    float cost = FLT_MAX;
    uint32_t best_bin = 0u, best_left = 0u;
    if (binning && lane < 3u && live[lane]) {
        const uint32_t *bins = s + 12u + lane * kSahBins * kBinWords;
        float right_cost[kSahBins];
        float alo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, ahi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        uint32_t cnt = 0u;
#pragma unroll
        for (int b = static_cast<int>(kSahBins) - 1; b > 0; --b) {
            const uint32_t *bin = bins + static_cast<uint32_t>(b) * kBinWords;
            for (int k = 0; k < 3; ++k) alo[k] = fminf(alo[k], lo_of(bin[k])), ahi[k] = fmaxf(ahi[k], hi_of(bin[3 + k]));
            cnt += bin[6];
            right_cost[b] = cnt ? half_area(alo, ahi) * static_cast<float>(cnt) : FLT_MAX;
        }
        for (int k = 0; k < 3; ++k) alo[k] = FLT_MAX, ahi[k] = -FLT_MAX;
        cnt = 0u;
#pragma unroll
        for (int b = 0; b < static_cast<int>(kSahBins) - 1; ++b) {
            const uint32_t *bin = bins + static_cast<uint32_t>(b) * kBinWords;
            for (int k = 0; k < 3; ++k) alo[k] = fminf(alo[k], lo_of(bin[k])), ahi[k] = fmaxf(ahi[k], hi_of(bin[3 + k]));
            cnt += bin[6];
            if (cnt == 0u || right_cost[b + 1] == FLT_MAX) continue;
            const float c = half_area(alo, ahi) * static_cast<float>(cnt) + right_cost[b + 1];
            if (c < cost) cost = c, best_bin = static_cast<uint32_t>(b) + 1u, best_left = cnt;
        }
    }
    float best_cost = FLT_MAX;
    int best_axis = -1;
    uint32_t bin = 0u, left = 0u;
    for (int a = 0; a < 3; ++a) {  // the first strict minimum in (axis, bin) order
        const float c = __shfl(cost, a);
        const uint32_t bb = __shfl(best_bin, a), bl = __shfl(best_left, a);
        if (c < best_cost) best_cost = c, best_axis = a, bin = bb, left = bl;
    }
    if (lane != 0u || j >= m) return;
    uint32_t kind = kKindLeaf, axis = 0u;
    if (active) {
        const float leaf_cost = half_area(blo, bhi) * static_cast<float>(count);
        const bool wanted = best_axis >= 0 && best_cost < leaf_cost;
        if (wanted && left > 0u && left < count) kind = kKindBinned, axis = static_cast<uint32_t>(best_axis);
        else if (wanted || count > kSahMaxLeaf) {
            kind = kKindMedian;
            float widest = -1.0f;
            for (uint32_t a = 0; a < 3u; ++a) {
                const float e = chi[a] - clo[a];
                if (e > widest) widest = e, axis = a;
            }
            left = count / 2u, bin = 0u;
        }
    }
    nflags[j] = kind != kKindLeaf ? 1u : 0u;
    if (j == m - 1u) nflags[m] = 0u;  // the scan runs over one word more than the level has nodes
    dec[j] = kind | (axis << 2) | (bin << 4);
    dlo[j] = clo[axis], dscale[j] = scale[axis];
    nleft[j] = left;
    if (kind == kKindLeaf) atomicMax(&counters[kBuildMaxLeaf], count);
    if (kind == kKindMedian) atomicAdd(&counters[kSahMedianTris], count);
}

// (d) behind the scan of the flags: child ranges, the next level's large slots, head words (the shape of rvpt_build.hip: emit_level)
__global__ void sah_emit(const uint2 *__restrict__ ranges, const uint32_t *__restrict__ nflags, const uint32_t *__restrict__ offs, const uint32_t *__restrict__ nleft, uint32_t n,
                         uint32_t begin, uint32_t m, uint32_t next_begin, uint2 *__restrict__ ranges_next, uint32_t *__restrict__ nslot_next, float4 *__restrict__ nodes,
                         uint32_t node_cap, uint32_t *__restrict__ counters)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m || begin + j >= node_cap) return;
    const uint2 r = ranges[j];
    const uint32_t off = offs[j], splits = nflags[j];
    uint32_t first = r.x, cnt = r.y;
    if (splits) {
        const uint32_t nl = nleft[j];
        first = next_begin + 2u * off, cnt = 0u;
        if (2u * off + 1u <= n && nl > 0u && nl < r.y) {  // (a level has at most n nodes; the host fails a build whose levels do not add up)
            const uint32_t c[2] = {nl, r.y - nl};
            ranges_next[2u * off] = make_uint2(r.x, c[0]);
            ranges_next[2u * off + 1u] = make_uint2(r.x + nl, c[1]);
            for (uint32_t k = 0; k < 2u; ++k) nslot_next[2u * off + k] = c[k] > kSahLargeNode ? atomicAdd(&counters[kSahLargeNext], 1u) : kNone;
        }
    }
    if (j == m - 1u) counters[kSahSplits] = off + splits;
    nodes[2u * (begin + j)] = make_float4(__uint_as_float(first), __uint_as_float(cnt), 0.f, 0.f);
    nodes[2u * (begin + j) + 1u] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// (c) per position: "goes left" of a binned node, "is sorted" of a median node; the scans run over one word more
__global__ void sah_flags(const float *__restrict__ tri, uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ pnode, uint32_t m, const uint32_t *__restrict__ dec,
                          const float *__restrict__ dlo, const float *__restrict__ dscale, uint32_t *__restrict__ pflag, uint32_t *__restrict__ mflag)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n) return;
    uint32_t left = 0u, sorted = 0u;
    if (p < n) {
        const uint32_t j = pnode[p], ti = idx[p];
        if (j < m && ti < n) {
            const uint32_t d = dec[j], kind = d & 3u, axis = (d >> 2) & 3u;
            if (kind == kKindBinned && axis < 3u) left = bin_of(tri[(6u + axis) * static_cast<size_t>(n) + ti], dlo[j], dscale[j]) < static_cast<int>(d >> 4) ? 1u : 0u;
            sorted = kind == kKindMedian ? 1u : 0u;
        }
    }
    pflag[p] = left;
    mflag[p] = sorted;
}

// the stable partition: a left triangle to begin + rank, a right one to begin + n_left + (pos - rank), the rank relative to the scan value at the node's begin;
// triangles of leaves and of nodes that are done are copied across; median nodes are written by sah_median_write
__global__ void sah_scatter(uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ pnode, uint32_t m, const uint2 *__restrict__ ranges,
                            const uint32_t *__restrict__ dec, const uint32_t *__restrict__ nleft, const uint32_t *__restrict__ offs, const uint32_t *__restrict__ pflag,
                            const uint32_t *__restrict__ prank, uint32_t *__restrict__ idx_out, uint32_t *__restrict__ pnode_out)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t j = pnode[p];
    const uint32_t kind = j < m ? (dec[j] & 3u) : kKindLeaf;
    if (kind == kKindMedian) return;
    uint32_t q = p, child = kNone;
    if (kind == kKindBinned) {
        const uint2 r = ranges[j];
        const uint32_t nl = nleft[j];
        if (r.x > p || r.x >= n) return;
        const uint32_t rank = prank[p] - prank[r.x], goes_left = pflag[p];
        q = goes_left ? r.x + rank : r.x + nl + ((p - r.x) - rank);
        child = 2u * offs[j] + (goes_left ? 0u : 1u);
        if (q >= n || q - r.x >= r.y) return;  // (cannot be: the counts of the bins and the flags are the same function of the same numbers)
    }
    idx_out[q] = idx[p];
    pnode_out[q] = child;
}

// median nodes: their positions compacted in order; the first sort is by caller's index, the second (stable) by (node of the level, centroid as an ordered
// integer with -0 canonical and a NaN on top)
__global__ void sah_median_compact(const float *__restrict__ tri, uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ pnode, uint32_t m,
                                   const uint32_t *__restrict__ dec, const uint32_t *__restrict__ mflag, const uint32_t *__restrict__ mrank, uint32_t n_median,
                                   uint32_t *__restrict__ cpos, uint32_t *__restrict__ key32, uint64_t *__restrict__ key64)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !mflag[p]) return;
    const uint32_t k = mrank[p], j = pnode[p], ti = idx[p];
    if (k >= n_median || j >= m || ti >= n) return;
    const uint32_t axis = min((dec[j] >> 2) & 3u, 2u);
    const float c = tri[(6u + axis) * static_cast<size_t>(n) + ti];
    const uint32_t e = c != c ? 0xFFFFFFFFu : ordered(c == 0.0f ? 0.0f : c);
    cpos[k] = p;
    key32[k] = ti;
    key64[k] = (static_cast<uint64_t>(j) << 32) | e;
}

__global__ void sah_median_write(uint32_t n, const uint32_t *__restrict__ cpos, const uint32_t *__restrict__ sorted, const uint64_t *__restrict__ keys, uint32_t n_median, uint32_t m,
                                 const uint2 *__restrict__ ranges, const uint32_t *__restrict__ nleft, const uint32_t *__restrict__ offs, uint32_t *__restrict__ idx_out,
                                 uint32_t *__restrict__ pnode_out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_median) return;
    const uint32_t p = cpos[k], j = static_cast<uint32_t>(keys[k] >> 32);
    if (p >= n || j >= m) return;
    const uint2 r = ranges[j];
    if (p < r.x || p - r.x >= r.y) return;  // (the k-th of the sorted triangles belongs to the node of the k-th compacted position: both are in node order)
    idx_out[p] = sorted[k];
    pnode_out[p] = 2u * offs[j] + ((p - r.x) < nleft[j] ? 0u : 1u);
}

// stage 3 from a plain index array: the 64-byte records gathered into leaf order, one thread per quad
__global__ void gather_records_by_index(const float4 *__restrict__ src, const uint32_t *__restrict__ order, uint32_t n_tris, float4 *__restrict__ out, uint32_t *__restrict__ perm)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t j = t >> 2, q = t & 3u;
    if (j >= n_tris) return;
    const uint32_t i = order[j];
    if (i >= n_tris) return;
    out[4u * j + q] = src[4u * i + q];
    if (q == 0u) perm[j] = i;
}

}  // namespace

size_t sah_scratch_bytes(uint32_t n)
{
    size_t total = 0;
    unsigned char origin[16];  // (only offsets are taken)
    carve(origin, n, &total);
    return total;
}

hipError_t sah_temp_bytes(uint32_t n, size_t *bytes)
{
    size_t a = 0, b = 0, c = 0;
    uint32_t *u = nullptr;
    uint64_t *k = nullptr;
    hipError_t e = rocprim::exclusive_scan(nullptr, a, u, u, 0u, static_cast<size_t>(n) + 1u, rocprim::plus<uint32_t>(), hipStream_t(nullptr));
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, b, u, u, k, k, n, 0, 32, hipStream_t(nullptr));
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(nullptr, c, k, k, u, u, n, 0, 64, hipStream_t(nullptr));
    if (e != hipSuccess) return e;
    *bytes = std::max(a, std::max(b, c));
    return hipSuccess;
}

hipError_t sah_begin(hipStream_t stream, const float4 *src, uint32_t n, unsigned char *scratch, uint32_t *counters, float4 *nodes)
{
    const Scratch s = carve(scratch, n);
    hipLaunchKernelGGL(sah_init, dim3(blocks_for(n)), dim3(kThreads), 0, stream, src, n, s.tri, s.idx[0], s.pnode[0], s.ranges[0], s.nslot[0], counters, nodes);
    return hipGetLastError();
}

hipError_t sah_decide_level(hipStream_t stream, void *temp, size_t temp_bytes, unsigned char *scratch, uint32_t n, uint32_t parity, uint32_t depth, uint32_t begin, uint32_t count,
                            uint32_t next_begin, uint32_t large_base, uint32_t n_large, float4 *nodes, uint32_t node_cap, uint32_t *counters)
{
    const Scratch s = carve(scratch, n);
    const uint32_t a = parity & 1u, b = a ^ 1u;
    n_large = std::min(n_large, s.large_cap);
    if (n_large) {
        const uint32_t windows = (n + kSahChunk - 1u) / kSahChunk;
        hipLaunchKernelGGL(sah_large_reset, dim3(blocks_for(n_large * kNodeWords)), dim3(kThreads), 0, stream, s.lbins, n_large);
        hipLaunchKernelGGL(sah_large_bounds, dim3(windows), dim3(kThreads), 0, stream, s.tri, n, s.idx[a], s.pnode[a], s.nslot[a], count, large_base, n_large, s.lbins);
        if (depth < kSahBalanceDepth)
            hipLaunchKernelGGL(sah_large_bins, dim3(windows), dim3(kThreads), 0, stream, s.tri, n, s.idx[a], s.pnode[a], s.nslot[a], count, large_base, n_large, s.lbins);
    }
    hipLaunchKernelGGL(sah_decide, dim3((count + kWavesPerGroup - 1u) / kWavesPerGroup), dim3(kThreads), 0, stream, s.tri, n, s.idx[a], s.ranges[a], s.nslot[a], s.lbins, large_base,
                       n_large, count, depth, s.nflags, s.dec, s.dlo, s.dscale, s.nleft, counters);
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, s.nflags, s.offs, 0u, static_cast<size_t>(count) + 1u, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sah_emit, dim3(blocks_for(count)), dim3(kThreads), 0, stream, s.ranges[a], s.nflags, s.offs, s.nleft, n, begin, count, next_begin, s.ranges[b], s.nslot[b], nodes,
                       node_cap, counters);
    return hipGetLastError();
}

hipError_t sah_partition_level(hipStream_t stream, void *temp, size_t temp_bytes, unsigned char *scratch, uint32_t n, uint32_t parity, uint32_t count, uint32_t n_median)
{
    const Scratch s = carve(scratch, n);
    const uint32_t a = parity & 1u, b = a ^ 1u;
    hipLaunchKernelGGL(sah_flags, dim3(blocks_for(n + 1u)), dim3(kThreads), 0, stream, s.tri, n, s.idx[a], s.pnode[a], count, s.dec, s.dlo, s.dscale, s.pflag, s.mflag);
    hipError_t e = rocprim::exclusive_scan(temp, temp_bytes, s.pflag, s.prank, 0u, static_cast<size_t>(n) + 1u, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sah_scatter, dim3(blocks_for(n)), dim3(kThreads), 0, stream, n, s.idx[a], s.pnode[a], count, s.ranges[a], s.dec, s.nleft, s.offs, s.pflag, s.prank, s.idx[b],
                       s.pnode[b]);
    if (n_median) {
        n_median = std::min(n_median, n);
        e = rocprim::exclusive_scan(temp, temp_bytes, s.mflag, s.mrank, 0u, static_cast<size_t>(n) + 1u, rocprim::plus<uint32_t>(), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(sah_median_compact, dim3(blocks_for(n)), dim3(kThreads), 0, stream, s.tri, n, s.idx[a], s.pnode[a], count, s.dec, s.mflag, s.mrank, n_median, s.cpos,
                           s.key32[0], s.key64[0]);
        e = rocprim::radix_sort_pairs(temp, temp_bytes, s.key32[0], s.key32[1], s.key64[0], s.key64[1], n_median, 0, 32, stream);
        if (e != hipSuccess) return e;
        e = rocprim::radix_sort_pairs(temp, temp_bytes, s.key64[1], s.key64[0], s.key32[1], s.key32[0], n_median, 0, 64, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(sah_median_write, dim3(blocks_for(n_median)), dim3(kThreads), 0, stream, n, s.cpos, s.key32[0], s.key64[0], n_median, count, s.ranges[a], s.nleft, s.offs,
                           s.idx[b], s.pnode[b]);
    }
    return hipGetLastError();
}

hipError_t sah_gather(hipStream_t stream, const float4 *src, const unsigned char *scratch, uint32_t n, uint32_t parity, float4 *tris_out, uint32_t *perm_out)
{
    const Scratch s = carve(const_cast<unsigned char *>(scratch), n);
    const uint64_t threads = 4ull * n;
    hipLaunchKernelGGL(gather_records_by_index, dim3(static_cast<uint32_t>((threads + kThreads - 1u) / kThreads)), dim3(kThreads), 0, stream, src, s.idx[parity & 1u], n, tris_out,
                       perm_out);
    return hipGetLastError();
}

}  // namespace rv
