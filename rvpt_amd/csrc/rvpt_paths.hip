// rvpt_paths.hip — path queries (include/rvpt_hip.h: RVPT_HIP_FORMAT_RAY_PATHS): a record comes in as a ray, an RNG state and a bounce budget and goes out as
// the radiance integrator_Kajiya (integrators.glsl:571-671) returns for that ray, with the number of segments the path traced, in place.
//
// The functions are the frame kernels', unchanged (rvpt_device.h): per segment the closest hit — the ray queries' walks (rvpt_query.hip) with the interval
// (0, +inf) —, then shade(), then shade's `bounce >= max_bounces` test against the RECORD's budget.  What a frame's mode-9 pixel evaluates after its camera ray
// is made, from a record instead of from a pixel.
//
// One path per lane, and REGENERATION: paths end after 1 .. max_bounces segments, so a lane whose path has ended stores its 16 out bytes and takes the next
// record of the run its wave has claimed (runs of kPathRun consecutive records off one counter; ballot / mbcnt hand-out as WavePool deals pixels) before the
// next segment's walk.  All three kernels run on a PERSISTENT grid sized from occupancy.  A record's answer is a function of its 32 in bytes and the scene
// alone: which lane or wave traced it, and beside which other records, changes nothing.
//
// GENERIC instances (RVPT_HIP_FORMAT_RAY_PATHS_MODE(0 .. 8)): the same kernels with shade_generic() where the lean ones have shade().  The mode belongs to the
// launch and sits in an SGPR; the continuation state (phase, ao_i, ao_acc, aux_o, aux_n) is per lane and exists only in the instance of the modes that ask
// further queries (PathForm below: HIT_ONLY for modes 0 .. 4, CONTINUING for 5 .. 8).  Lanes of one wave sit
// in different phases — a main segment beside a shadow query beside an occlusion sample —, and every phase asks the same question, the closest hit in (0, +inf);
// so regeneration is unchanged, and a record's answer is a function of its 32 in bytes, the call's mode and the scene.  Hart is not built.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rvpt_device.h"
#include "rvpt_paths.h"
#include "rvpt_walk.h"

namespace rv {

namespace {

constexpr uint32_t kNoPrim = 0xFFFFFFFFu;

struct PathArgs {
    const float4 *prep, *nodes, *wide, *unit_n, *mats;
    const uint32_t *mat_index;
    float4 *records;
    uint32_t n, n_runs;          // records, runs of kPathRun records
    uint32_t *counter;           // the next run to claim (0 at launch)
    uint32_t *stack_overflow;    // [stack_levels - lds_levels][2][threads of the grid]
    uint32_t n_tris, head_shift, stack_levels, lds_levels, top_nodes;
    uint32_t mode;               // GENERIC instances: the call's integrator, render mode 0 .. 8 of compute_pass.comp:76-95 (the lean instances are mode 9 and do not read it)
};

// The path a lane is tracing: the frame kernels' Lane (segment, throughput, radiance so far, RNG state, finished segments) with the record it came from
struct PathLane {
    Lane L;
    uint32_t rec;     // index of the record
    int max_bounces;  // the record's budget, 1 .. kPathMaxBounces
    bool have;        // false: this lane holds no path
};

// The records of the run a wave has claimed and not yet dealt (wave-uniform)
struct RunPool {
    uint32_t next = 0, end = 0;
    bool exhausted = false;  // the counter has passed the last run
};

// The instances of each kernel.  LEAN is integrator_Kajiya under shade(), the code of RVPT_HIP_FORMAT_RAY_PATHS.  The GENERIC instances run shade_generic() and
// are two: HIT_ONLY for the modes that end at the first hit (0 .. 4: no continuation state, no RNG use) and CONTINUING for those that ask further queries (5 .. 8).
// One GENERIC instance for all nine modes cost path_bvh4 a work-group per CU against the lean one (89 VGPRs: five waves per SIMD where 74 allow six); the split
// keeps that cost to the modes whose state needs the registers (profiles/path_modes.txt has both sets of figures).
enum PathForm { LEAN = 0, HIT_ONLY = 1, CONTINUING = 2 };

// The integrator of a GENERIC launch: a kernel argument, so one value for the whole wave, held in an SGPR — shade_generic's switch on it is a scalar branch.
// The host launches an instance with the modes of its form only; the clamp tells the compiler so: the other forms' cases and shade_generic's default branch
// (hart(), which would read tris the path kernels are not given) are not built into it.
template <int FORM>
__device__ __forceinline__ uint32_t path_mode(const PathArgs &a)
{
    return FORM == HIT_ONLY ? min(a.mode, 4u) : max(5u, min(a.mode, 8u));
}

__device__ __forceinline__ bool finite_(const float x) { return __builtin_fabsf(x) < kInf; }  // false for NaN and +-inf

// Every lane without a path takes the next record of the wave's run, in lane order; the wave claims a new run when the one it holds is dealt.  An invalid
// record — a non-finite component of org or dir, a budget of 0 or past kPathMaxBounces — is answered here, before any walk: radiance 0, segments 0.
// On return a lane without a path means that the records are all dealt.
// CONTINUING: a record starts as begin_sample_generic leaves a sample after the camera — the main phase, and integrator_Whitted's ambient term (integrators.glsl:293)
// in col.  The continuation state of the record before it on the lane needs no reset: shade_generic writes aux_o, aux_n, ao_acc and ao_i when it enters PH_AO.
template <int FORM>
__device__ __forceinline__ void regenerate_paths(RunPool &pool, const PathArgs &a, const uint32_t lane, PathLane &P)
{
    bool need = !P.have;
    for (;;) {
        const uint64_t mask = ballot(need);
        if (mask == 0) break;
        uint32_t avail = pool.end - pool.next;
        if (avail == 0) {
            if (pool.exhausted) break;
            uint32_t run = 0;
            if (lane == 0) run = atomicAdd(a.counter, 1u);
            run = __builtin_amdgcn_readlane(run, 0);
            if (run >= a.n_runs) {
                pool.exhausted = true;
                break;
            }
            pool.next = run * kPathRun;  // (< n <= 2^32 - 1)
            avail = min(kPathRun, a.n - pool.next);
            pool.end = pool.next + avail;
        }
        const uint32_t rank = prefix_rank(mask);
        const uint32_t wanted = static_cast<uint32_t>(__builtin_popcountll(mask));
        if (need && rank < avail) {
            const size_t r = static_cast<size_t>(pool.next) + rank;
            const float4 ra = a.records[3 * r + 0];
            const float4 rb = a.records[3 * r + 1];
            const uint32_t budget = __float_as_uint(rb.w);
            const bool valid = finite_(ra.x) && finite_(ra.y) && finite_(ra.z) && finite_(rb.x) && finite_(rb.y) && finite_(rb.z) && budget >= 1u && budget <= kPathMaxBounces;
            if (valid) {
                P.L.o = mk(ra.x, ra.y, ra.z);
                P.L.d = mk(rb.x, rb.y, rb.z);
                P.L.thr = mk(1.0f, 1.0f, 1.0f);
                P.L.col = mk(0.0f, 0.0f, 0.0f);
                if (FORM == CONTINUING) {
                    const float ambient = (path_mode<FORM>(a) == 7u) ? 0.1f : 0.0f;
                    P.L.col = mk(ambient, ambient, ambient);
                    P.L.phase = PH_MAIN;
                }
                P.L.rng = __float_as_uint(ra.w);
                P.L.bounce = 0;
                P.L.nseg = 0;
                P.rec = static_cast<uint32_t>(r);
                P.max_bounces = static_cast<int>(budget);
                P.have = true;
                need = false;
            } else {
                a.records[3 * r + 2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        pool.next += min(wanted, avail);
    }
}

// A finished segment: shade() as a frame runs it, with the record's budget where a frame has its settings'.  A path that ended stores its out fields — the
// integrator's value itself (a frame adds it to zero), the segments it traced — and frees the lane.  Returns true when the path goes on with L.o, L.d.
// GENERIC forms: shade_generic() with the launch's mode, for the phase the lane is in: a shadow query or an occlusion sample is a segment like any other, and the
// record's budget is also what PH_AO reads as its sample count.
template <int FORM>
__device__ __forceinline__ bool finish_segment(const PathArgs &a, const ShadeSrc src, PathLane &P, const uint32_t hit, const float closest)
{
    FrameParams fp;  // shade() and shade_generic() read their bounce budget and nothing else
    fp.max_bounces = P.max_bounces;
    if (FORM != LEAN) P.L.mode = static_cast<int>(path_mode<FORM>(a));
    if (FORM == HIT_ONLY) P.L.phase = PH_MAIN;  // (these modes never leave it)
    f3 radiance = mk(0.0f, 0.0f, 0.0f);
    P.L.nseg += 1;
    if (!shade_t<FORM != LEAN>(P.L, fp, src, hit, closest, radiance)) return true;
    a.records[3 * static_cast<size_t>(P.rec) + 2] = make_float4(radiance.x, radiance.y, radiance.z, __uint_as_float(P.L.nseg));
    P.have = false;
    return false;
}

enum { S_IDLE = 0, S_TRAV = 1, S_HIT = 2 };  // no segment / a segment whose walk is to start or under way / a segment whose closest hit is known

}  // namespace

// The 4-wide walk of rvpt_walk.h (walk_bvh4's: its order, its stack and its LDS layout are stated there) under the frame kernel's loop: lanes whose walk has
// ended wait in S_HIT until kPathRefill of them do, then shade, regenerate and start the next walk together; reached leaves are parked and run in batches.
template <int FORM>
__global__ __launch_bounds__(kBlock) void path_bvh4(const PathArgs a)
{
    const WideTree tree(a.lds_levels, a.nodes, a.wide, a.top_nodes, a.head_shift);
    const WalkStack<2> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const ShadeSrc shade_src{a.prep, a.mat_index, a.mats, a.unit_n};
    const uint32_t lane = lane_id();

    RunPool pool;
    PathLane P{};
    int state = S_IDLE;
    bool walking = false;
    float closest = kInf;
    uint32_t hit = kNoPrim, sp = 0;
    WideAt at;
    f3 inv = mk(0.0f, 0.0f, 0.0f);

    for (;;) {
        // ---- refill: every lane that is not walking shades the segment it finished, takes a record if its path ended, and starts its next walk
        for (;;) {
            if (state == S_HIT) state = finish_segment<FORM>(a, shade_src, P, hit, closest) ? S_TRAV : S_IDLE;
            regenerate_paths<FORM>(pool, a, lane, P);
            if (P.have && state == S_IDLE) state = S_TRAV;
            if (state == S_TRAV && !walking) {  // start at the root: its own box first (the root is a node like any other, intersection.glsl:369-380)
                closest = kInf;
                hit = kNoPrim;
                inv = mk(1.0f / P.L.d.x, 1.0f / P.L.d.y, 1.0f / P.L.d.z);
                sp = 0;
                float entry;
                if (slab_entry(P.L.o, inv, tree.lds_root[0], tree.lds_root[1], closest, entry)) {
                    at.cur = 0;  // the wide root
                    at.leaf_count = 0;
                    walking = true;
                } else {
                    state = S_HIT;
                }
            }
            if (ballot(state == S_HIT) == 0) break;  // (a ray that misses the root's box is a finished segment: round again)
        }
        if (ballot(state == S_TRAV) == 0) break;  // no lane walks: none holds a path, and none is left to deal

        // ---- traverse: every iteration each walking lane handles one wide node; leaves are parked and run in batches
        for (uint32_t steps = 0;; ++steps) {
            bool need_pop = false;
            if (state == S_TRAV && at.leaf_count == 0) wide_step(tree, P.L.o, inv, closest, stack, sp, at, need_pop);
            const uint32_t at_leaf = static_cast<uint32_t>(__builtin_popcountll(ballot(at.leaf_count > 0)));
            const uint32_t at_inner = static_cast<uint32_t>(__builtin_popcountll(ballot(state == S_TRAV && at.leaf_count == 0)));
            const bool run_leaves = at_leaf > 0 && (at_inner == 0 || at_leaf >= kPathLeafBatch);
            if (run_leaves && at.leaf_count > 0) {
                for (uint32_t i = at.leaf_first; i < at.leaf_first + at.leaf_count; ++i) {
                    const v4f *tp = prep + 4 * static_cast<size_t>(i);
                    test_triangle(unpack(tp[0], tp[1], tp[2], tp[3]), P.L.o, P.L.d, i, closest, hit);
                }
                at.leaf_count = 0;
                need_pop = true;
            }
            if (need_pop && !wide_pop(tree, closest, stack, sp, at)) {
                state = S_HIT;
                walking = false;
            }
            if (ballot(state == S_TRAV) == 0) break;
            const uint32_t waiting = static_cast<uint32_t>(__builtin_popcountll(ballot(state == S_HIT)));
            if (waiting >= kPathRefill || (waiting > 0 && steps >= 4u * kPathRefill)) break;
        }
    }
}

// walk_bvh2's walk (rvpt_query.hip) — intersect_bvh as the reference writes it, over the binary nodes: pop a node, test its box against the interval of that moment, a leaf's
// triangles in order, an inner node's right child stacked and its left child next — under the same loop.  One word per stack slot (the node index).
template <int FORM>
__global__ __launch_bounds__(kBlock) void path_bvh2(const PathArgs a)
{
    const WalkStack<1> stack(a.lds_levels, a.stack_levels, a.stack_overflow);
    const v4f *prep = reinterpret_cast<const v4f *>(a.prep);
    const ShadeSrc shade_src{a.prep, a.mat_index, a.mats, a.unit_n};
    const uint32_t lane = lane_id();

    RunPool pool;
    PathLane P{};
    int state = S_IDLE;
    bool walking = false;
    float closest = kInf;
    uint32_t hit = kNoPrim, sp = 0, cur = 0;
    f3 inv = mk(0.0f, 0.0f, 0.0f);

    for (;;) {
        for (;;) {
            if (state == S_HIT) state = finish_segment<FORM>(a, shade_src, P, hit, closest) ? S_TRAV : S_IDLE;
            regenerate_paths<FORM>(pool, a, lane, P);
            if (P.have && state == S_IDLE) state = S_TRAV;
            if (state == S_TRAV && !walking) {  // (the root's box is tested by the first step below, as every node's)
                closest = kInf;
                hit = kNoPrim;
                inv = mk(1.0f / P.L.d.x, 1.0f / P.L.d.y, 1.0f / P.L.d.z);
                sp = 0;
                cur = 0;
                walking = true;
            }
            if (ballot(state == S_HIT) == 0) break;
        }
        if (ballot(state == S_TRAV) == 0) break;

        for (uint32_t steps = 0;; ++steps) {
            if (state == S_TRAV) {
                const float4 n0 = a.nodes[2u * static_cast<size_t>(cur)], n1 = a.nodes[2u * static_cast<size_t>(cur) + 1u];
                const uint32_t first = __float_as_uint(n0.x), count = __float_as_uint(n0.y);
                bool pop = true;
                float entry;
                if (slab_entry(P.L.o, inv, n0, n1, closest, entry)) {
                    if (count > 0) {
                        for (uint32_t i = first; i < first + count; ++i) {
                            const v4f *tp = prep + 4 * static_cast<size_t>(i);
                            test_triangle(unpack(tp[0], tp[1], tp[2], tp[3]), P.L.o, P.L.d, i, closest, hit);
                        }
                    } else {
                        stack.push(sp, first + 1u);  // (the tree's height bounds the pushes of a root-to-leaf path)
                        cur = first;
                        pop = false;
                    }
                }
                if (pop) {
                    if (sp == 0) {
                        state = S_HIT;
                        walking = false;
                    } else {
                        cur = stack.pop(sp);
                    }
                }
            }
            if (ballot(state == S_TRAV) == 0) break;
            const uint32_t waiting = static_cast<uint32_t>(__builtin_popcountll(ballot(state == S_HIT)));
            if (waiting >= kPathRefill || (waiting > 0 && steps >= 4u * kPathRefill)) break;
        }
    }
}

// Brute force, in work-group-synchronous ROUNDS: at a round's start every lane without a path takes a record (each wave deals its own runs); then the prepared
// triangles stream through LDS in tiles of kQueryTileTris, as walk_brute streams them, and every lane that holds a path runs its current segment over each
// tile in index order; then it shades.  The work-group leaves when a round starts with no path in any of its lanes.  No culls: the packet kernel's rest on a
// camera and a block of pixels.
template <int FORM>
__global__ __launch_bounds__(kBlock) void path_brute(const PathArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds_tile[];
    const ShadeSrc shade_src{a.prep, a.mat_index, a.mats, a.unit_n};
    const uint32_t lane = lane_id();
    RunPool pool;
    PathLane P{};
    for (;;) {
        regenerate_paths<FORM>(pool, a, lane, P);
        if (__syncthreads_or(P.have ? 1 : 0) == 0) break;  // (also the barrier between the last round's tile reads and this round's tile stores)
        if (!P.have) P.L.d = mk(0.0f, 0.0f, 0.0f);  // a lane without a path runs along: every test of a zero direction is NaN and accepts nothing
        float closest = kInf;
        uint32_t hit = kNoPrim;
        const uint64_t wave_has = ballot(P.have);
        for (uint32_t base = 0; base < a.n_tris; base += kQueryTileTris) {
            const uint32_t count = min(kQueryTileTris, a.n_tris - base);
            if (base != 0) __syncthreads();  // the tile before this one has been read by every wave
            for (uint32_t i = threadIdx.x; i < 4u * count; i += kBlock) lds_tile[i] = a.prep[4u * static_cast<size_t>(base) + i];
            __syncthreads();
            if (wave_has != 0) intersect_run<4>(reinterpret_cast<const v4f *>(lds_tile), base, count, P.L.o, P.L.d, closest, hit);
        }
        if (P.have) (void)finish_segment<FORM>(a, shade_src, P, hit, closest);
    }
}

namespace {

template <int FORM>
const void *path_kernel_of(const QueryKind kind)
{
    if (kind == QueryKind::Brute) return reinterpret_cast<const void *>(path_brute<FORM>);
    return kind == QueryKind::Wide ? reinterpret_cast<const void *>(path_bvh4<FORM>) : reinterpret_cast<const void *>(path_bvh2<FORM>);
}

// The instance a launch runs: the lean one for integrator_Kajiya, a GENERIC one for the render modes 0 .. 8
const void *path_kernel(const QueryKind kind, const uint32_t mode)
{
    if (mode == kPathModeKajiya) return path_kernel_of<LEAN>(kind);
    return mode <= 4u ? path_kernel_of<HIT_ONLY>(kind) : path_kernel_of<CONTINUING>(kind);
}

}  // namespace

hipError_t path_plan(const PathScene &scene, const uint32_t n, const int num_cus, const uint32_t mode, QueryPlan *plan)
{
    if (mode > kPathModeKajiya) return hipErrorInvalidValue;
    QueryPlan p{};
    const QueryKind kind = scene.walk.kind;
    const void *kernel = path_kernel(kind, mode);  // the occupancy is the launched instance's own
    uint32_t levels = 0;
    if (kind == QueryKind::Brute) {
        p.lds_bytes = static_cast<size_t>(kQueryTileTris) * 64u;
    } else {
        levels = std::max<uint32_t>(1u, scene.walk.stack_levels);
        p.lds_levels = std::min(levels, kQueryLdsLevels);
        p.top_nodes = kind == QueryKind::Wide ? std::min(scene.walk.n_wide, kQueryTopNodes) : 0u;
        p.lds_bytes = static_cast<size_t>(p.lds_levels) * kBlock * 2u * sizeof(uint32_t) + 2u * sizeof(float4) + static_cast<size_t>(p.top_nodes) * 128u;
    }
    int per_cu = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, p.lds_bytes);
    if (e != hipSuccess) return e;
    const uint64_t runs = (static_cast<uint64_t>(n) + kPathRun - 1u) / kPathRun;
    const uint64_t want = (runs + kBlock / 64u - 1u) / (kBlock / 64u);  // a work-group's four waves claim a run each
    p.grid = static_cast<uint32_t>(std::max<uint64_t>(1u, std::min<uint64_t>(want, static_cast<uint64_t>(std::max(per_cu, 1)) * static_cast<uint64_t>(std::max(num_cus, 1)))));
    const size_t column_words = static_cast<size_t>(2u) * (levels - p.lds_levels) * kBlock;  // per work-group
    while (p.grid > 1u && column_words * p.grid * sizeof(uint32_t) > kQueryStackMaxBytes) p.grid = (p.grid + 1u) / 2u;
    p.stack_words = column_words * p.grid;
    *plan = p;
    return hipSuccess;
}

hipError_t path_launch(hipStream_t stream, const PathScene &scene, const QueryPlan &plan, uint32_t *scratch, void *records, const uint32_t n, const uint32_t mode)
{
    if (mode > kPathModeKajiya) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    PathArgs a{};
    a.prep = scene.walk.prep, a.nodes = scene.walk.nodes, a.wide = scene.walk.wide;
    a.unit_n = scene.unit_n, a.mats = scene.mats, a.mat_index = scene.mat_index;
    a.records = static_cast<float4 *>(records);
    a.n = n;
    a.n_runs = static_cast<uint32_t>((static_cast<uint64_t>(n) + kPathRun - 1u) / kPathRun);
    a.counter = scratch;
    a.stack_overflow = scratch + 64;
    a.n_tris = scene.walk.n_tris, a.head_shift = scene.walk.head_shift;
    a.stack_levels = std::max<uint32_t>(1u, scene.walk.stack_levels);
    a.lds_levels = plan.lds_levels, a.top_nodes = plan.top_nodes;
    a.mode = mode;
    const hipError_t e = hipMemsetAsync(scratch, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    void *kernel_args[] = {&a};
    return hipLaunchKernel(path_kernel(scene.walk.kind, mode), dim3(plan.grid), dim3(kBlock), kernel_args, plan.lds_bytes, stream);
}

}  // namespace rv
