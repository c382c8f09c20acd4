// rvpt_surface.hip — the geometry read-back (include/rvpt_hip.h: TRIANGLES and SURFACE POINTS at rvpt_hip_read).
//
// TRIANGLES: the 64-byte rows of d_tris as they stand, in the update order of the context.  Without a permutation that is d_tris itself and rvpt_abi.hip copies
// it; with one it is the row scatter out[perm[s]] = tris[s], which the guarded rebuild's carry-back already is: rv::carry_back_triangles (rvpt_refit.hip), one
// thread per 16-byte quad, coalesced reads, four neighbouring lanes writing one row.  It is launched from here, not restated.
//
// SURFACE POINTS: a record comes in as (prim, u, v) — a triangle in the queries' numbering and the pair a query reported — and goes out as the point
// (a + (b-a)*u) + (c-a)*v of the stored row, the normal prepare_triangles stored for it and its material word.  binary32, every operation rounded on its own:
// this translation unit is compiled with -ffp-contract=off like every other and there is no fma_() in it.  One record per lane: one float4 load of the in-quad,
// the three vertex quads, the normal's quad and the material word of the stored row, two float4 stores.  A prim read from a record becomes an address only
// below n_tris, and so does the row the inverse permutation gives for it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvpt_refit.h"
#include "rvpt_surface.h"

namespace rv {

namespace {

constexpr uint32_t kSurfaceBlock = 256;
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

struct SurfaceArgs {
    const float4 *tris, *unit_n;
    const uint32_t *mat_index, *inv_perm;
    float4 *records;
    uint32_t n, n_tris;
};

__device__ __forceinline__ bool finite_(const float x) { return __builtin_fabsf(x) < __builtin_inff(); }  // false for NaN and +-inf

__device__ __forceinline__ float along(const float a, const float b, const float c, const float u, const float v)
{
    const float ab = b - a, ac = c - a;
    return (a + ab * u) + ac * v;
}

}  // namespace

__global__ __launch_bounds__(kSurfaceBlock) void surface_points(const SurfaceArgs a)
{
    const size_t r = static_cast<size_t>(blockIdx.x) * kSurfaceBlock + threadIdx.x;
    if (r >= a.n) return;
    const float4 in = a.records[3u * r];
    const uint32_t prim = __float_as_uint(in.x);
    const float u = in.y, v = in.z;
    uint32_t row = kNoRow;
    if (prim < a.n_tris && finite_(u) && finite_(v)) row = a.inv_perm ? a.inv_perm[prim] : prim;
    float4 point = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu)), normal = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (row < a.n_tris) {
        const float4 va = a.tris[4u * static_cast<size_t>(row)], vb = a.tris[4u * static_cast<size_t>(row) + 1u], vc = a.tris[4u * static_cast<size_t>(row) + 2u];
        const float4 un = a.unit_n[row];
        point = make_float4(along(va.x, vb.x, vc.x, u, v), along(va.y, vb.y, vc.y, u, v), along(va.z, vb.z, vc.z, u, v), __uint_as_float(a.mat_index[row]));
        normal = make_float4(un.x, un.y, un.z, 0.0f);
    }
    a.records[3u * r + 1u] = point;
    a.records[3u * r + 2u] = normal;
}

hipError_t surface_scatter_rows(hipStream_t stream, const float4 *tris, const uint32_t *perm, const uint32_t n, void *out)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(carry_back_triangles, dim3(static_cast<uint32_t>((4ull * n + 255u) / 256u)), dim3(256), 0, stream, tris, perm, n, static_cast<float4 *>(out));
    return hipGetLastError();
}

hipError_t surface_launch(hipStream_t stream, const SurfaceScene &scene, void *records, const uint32_t n)
{
    if (n == 0) return hipSuccess;
    SurfaceArgs a{};
    a.tris = scene.tris, a.unit_n = scene.unit_n, a.mat_index = scene.mat_index, a.inv_perm = scene.inv_perm;
    a.records = static_cast<float4 *>(records);
    a.n = n, a.n_tris = scene.n_tris;
    hipLaunchKernelGGL(surface_points, dim3(static_cast<uint32_t>((static_cast<uint64_t>(n) + kSurfaceBlock - 1u) / kSurfaceBlock)), dim3(kSurfaceBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rv
