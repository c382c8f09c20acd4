// rvpt_walk.h — what the query walks share (rvpt_query.hip, rvpt_paths.hip, rvpt_nearest.hip, rvpt_box.hip): the split traversal stack, the claim of a run of
// records, the step and the pop of the 4-wide walk, the four-at-a-time run over an LDS tile, and the triangle test that also gives u and v.  Device code only;
// every function is inlined into the kernel that uses it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvpt_device.h"

namespace rv {

// A walking work-group's dynamic LDS; it begins with the stack.  WalkStack indexes the array itself: through a pointer member the compiler loses the address
// space at the pop and reads LDS with flat loads.
extern __shared__ __attribute__((aligned(16))) uint32_t walk_lds[];

// The traversal stack of one lane, WORDS words per slot, under the lane's own count `sp` of held slots: the first lds_levels slots in LDS, the deeper ones in
// one global column per thread of the grid.  LDS: [lds_levels][WORDS][kBlock] words, global: [stack_levels - lds_levels][WORDS][threads of the grid].  The host
// sizes the stack from the tree (the wide tree's stack levels, the binary tree's height), so sp never passes top_level; the clamp of push() keeps a wrong size
// inside the memory.
template <uint32_t WORDS>
struct WalkStack {
    uint32_t lds_levels, top_level;
    uint32_t *ovf;  // this thread's column
    size_t ovf_stride;

    __device__ __forceinline__ WalkStack(const uint32_t lds_levels_, const uint32_t stack_levels, uint32_t *stack_overflow)
        : lds_levels(lds_levels_), top_level(stack_levels - 1u), ovf(stack_overflow + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x)),
          ovf_stride(static_cast<size_t>(gridDim.x) * kBlock)
    {
    }
    // (a one-word stack takes and gives w0 alone)
    __device__ __forceinline__ void push(uint32_t &sp, const uint32_t w0, const uint32_t w1 = 0u) const
    {
        const uint32_t at = min(sp, top_level);
        if (at < lds_levels) {
            walk_lds[(WORDS * at + 0u) * kBlock + threadIdx.x] = w0;
            if (WORDS == 2) walk_lds[(WORDS * at + 1u) * kBlock + threadIdx.x] = w1;
        } else {
            ovf[(WORDS * (at - lds_levels) + 0u) * ovf_stride] = w0;
            if (WORDS == 2) ovf[(WORDS * (at - lds_levels) + 1u) * ovf_stride] = w1;
        }
        sp = at + 1u;
    }
    __device__ __forceinline__ void pop(uint32_t &sp, uint32_t &w0, uint32_t &w1) const  // sp > 0
    {
        sp -= 1;
        if (sp < lds_levels) {
            w0 = walk_lds[(WORDS * sp + 0u) * kBlock + threadIdx.x];
            if (WORDS == 2) w1 = walk_lds[(WORDS * sp + 1u) * kBlock + threadIdx.x];
        } else {
            w0 = ovf[(WORDS * (sp - lds_levels) + 0u) * ovf_stride];
            if (WORDS == 2) w1 = ovf[(WORDS * (sp - lds_levels) + 1u) * ovf_stride];
        }
    }
    __device__ __forceinline__ uint32_t pop(uint32_t &sp) const  // sp > 0
    {
        static_assert(WORDS == 1, "a two-word slot is popped into two words");
        sp -= 1;
        return sp < lds_levels ? walk_lds[sp * kBlock + threadIdx.x] : ovf[(sp - lds_levels) * ovf_stride];
    }
};

// the next run of records for this wave off the launch's counter (wave-uniform)
__device__ __forceinline__ uint32_t claim_run(uint32_t *counter, const uint32_t lane)
{
    uint32_t run = 0;
    if (lane == 0) run = atomicAdd(counter, 1u);
    return __builtin_amdgcn_readlane(run, 0);
}

// THE 4-WIDE WALK (rvpt_bvh4.hip's per-lane walk): slab_entry at the root, four slab_child tests per wide node, on with the first child that passes, the others
// stacked (the last first) with their entry distances and packed heads, popped with bound >= entry — the reference's box test at the visit, against the
// interval of that moment (rvpt_bvh4.hip's header comment).  The root's box and the first top_nodes wide nodes of the (breadth-first) tree are read from LDS,
// which holds them behind the stack: [stack: lds_levels x 2 words x kBlock][root: 2 float4][top_nodes wide nodes].
struct WideTree {
    const float4 *lds_root, *lds_top, *wide;
    uint32_t top_nodes, head_shift;

    // every thread of the work-group; ends in a barrier
    __device__ __forceinline__ WideTree(const uint32_t lds_levels, const float4 *nodes, const float4 *wide_, const uint32_t top_nodes_, const uint32_t head_shift_)
        : wide(wide_), top_nodes(top_nodes_), head_shift(head_shift_)
    {
        float4 *root = reinterpret_cast<float4 *>(walk_lds + 2u * lds_levels * kBlock);
        float4 *top = root + 2;
        if (threadIdx.x < 2u) root[threadIdx.x] = nodes[threadIdx.x];
        for (uint32_t i = threadIdx.x; i < 8u * top_nodes; i += kBlock) top[i] = wide[i];
        __syncthreads();
        lds_root = root;
        lds_top = top;
    }
};

// Where a lane of the wide walk stands: at wide node `cur` (leaf_count 0) or in front of a leaf's triangles
struct WideAt {
    uint32_t cur = 0, leaf_first = 0, leaf_count = 0;

    __device__ __forceinline__ void enter(const uint32_t head, const uint32_t head_shift)  // head = first | count << head_shift (leaf, count > 0) or a wide node index (count 0)
    {
        const uint32_t first = head & ((1u << head_shift) - 1u), count = head >> head_shift;
        cur = first;
        leaf_first = first;
        leaf_count = count;
    }
};

// One wide node: need_pop is set when no child passes
__device__ __forceinline__ void wide_step(const WideTree &tree, const f3 o, const f3 inv, const float bound, const WalkStack<2> &stack, uint32_t &sp, WideAt &at, bool &need_pop)
{
    const float4 *node = at.cur < tree.top_nodes ? tree.lds_top + 8u * at.cur : tree.wide + 8u * static_cast<size_t>(at.cur);
    const float4 minx = node[0], maxx = node[1], miny = node[2], maxy = node[3], minz = node[4], maxz = node[5], hq = node[6];
    const uint32_t hd0 = __float_as_uint(hq.x), hd1 = __float_as_uint(hq.y), hd2 = __float_as_uint(hq.z), hd3 = __float_as_uint(hq.w);
    float e0, e1, e2, e3;
    const bool h0 = slab_child(o, inv, minx.x, maxx.x, miny.x, maxy.x, minz.x, maxz.x, bound, e0);  // (a wide node has at least two children)
    const bool h1 = slab_child(o, inv, minx.y, maxx.y, miny.y, maxy.y, minz.y, maxz.y, bound, e1);
    const bool h2 = slab_child(o, inv, minx.z, maxx.z, miny.z, maxy.z, minz.z, maxz.z, bound, e2) && hd2 != kWideEmpty;
    const bool h3 = slab_child(o, inv, minx.w, maxx.w, miny.w, maxy.w, minz.w, maxz.w, bound, e3) && hd3 != kWideEmpty;
    if (h3 && (h0 || h1 || h2)) stack.push(sp, __float_as_uint(e3), hd3);
    if (h2 && (h0 || h1)) stack.push(sp, __float_as_uint(e2), hd2);
    if (h1 && h0) stack.push(sp, __float_as_uint(e1), hd1);
    if (h0 || h1 || h2 || h3)
        at.enter(h0 ? hd0 : (h1 ? hd1 : (h2 ? hd2 : hd3)), tree.head_shift);
    else
        need_pop = true;
}

// The next stacked child whose entry distance the bound still reaches: false when the stack runs out (the walk is over)
__device__ __forceinline__ bool wide_pop(const WideTree &tree, const float bound, const WalkStack<2> &stack, uint32_t &sp, WideAt &at)
{
    bool found = false;
    while (sp > 0 && !found) {
        uint32_t entry_bits, head;
        stack.pop(sp, entry_bits, head);
        if (bound >= __uint_as_float(entry_bits)) {
            at.enter(head, tree.head_shift);
            found = true;
        }
    }
    return found;
}

// test_triangle's arithmetic (rvpt_device.h) with u and v kept: the same operations on the same operands, hence the same bits
struct TriangleUV {
    float tt, u, v;
};
__device__ __forceinline__ TriangleUV test_triangle_uv(const PrepTri &t, const f3 o, const f3 d)
{
    TriangleUV r;
    r.tt = div_dots(dot(t.v0 - o, t.n), dot(d, t.n));
    const f3 p0 = fma3(d, r.tt, o) - t.v0;
    const float b0 = dot(p0, t.e0);
    const float b1 = dot(p0, t.e1);
    r.u = t.inv_det * fma_(t.a01, b1, t.a00 * b0);
    r.v = t.inv_det * fma_(t.a11, b1, t.a01 * b0);
    return r;
}

// intersect_run<4> (rvpt_device.h) with the caller's accept: `count` consecutive prepared triangles at `src` (LDS), indices index0, index0 + 1, ...; four
// tests' arithmetic is scheduled together (the empty asm consumes all their results), then accept(test, index) runs for the four in order.
template <class Accept>
__device__ __forceinline__ void tile_run(const v4f *src, const uint32_t index0, const uint32_t count, const f3 o, const f3 d, Accept accept)
{
    uint32_t i = 0;
    for (; i + 4 <= count; i += 4) {
        OpenTest r[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t j = i + k;
            r[k] = test_triangle_open(unpack(src[4 * j + 0], src[4 * j + 1], src[4 * j + 2], src[4 * j + 3]), o, d);
        }
        asm volatile("" ::"v"(r[0].tt), "v"(r[0].m), "v"(r[0].s), "v"(r[1].tt), "v"(r[1].m), "v"(r[1].s), "v"(r[2].tt), "v"(r[2].m), "v"(r[2].s), "v"(r[3].tt),
                     "v"(r[3].m), "v"(r[3].s));
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) accept(r[k], index0 + i + k);
    }
    for (; i < count; ++i) accept(test_triangle_open(unpack(src[4 * i + 0], src[4 * i + 1], src[4 * i + 2], src[4 * i + 3]), o, d), index0 + i);
}

}  // namespace rv
