// rvpt_surface.h — the geometry read-back (include/rvpt_hip.h: RVPT_HIP_FORMAT_TRIANGLES, RVPT_HIP_FORMAT_SURFACE_POINTS): the stored triangle rows in update
// order, and points on the stored mesh for a caller's (prim, u, v).  The kernels live in rvpt_surface.hip (the row scatter is rvpt_refit.hip's
// carry_back_triangles, launched from there); rvpt_abi.hip validates, stages host memory and owns the buffers.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rv {

constexpr uint32_t kSurfaceRecordBytes = 48;  // sizeof(rvpt_surface_point): three float4

// What a surface record reads: the rows every update form keeps current
struct SurfaceScene {
    const float4 *tris;         // n_tris x 4 float4: rvpt_triangle rows (d_tris), of which vert0..2 are read
    const float4 *unit_n;       // n_tris float4: the normal prepare_triangles stored, w = 0
    const uint32_t *mat_index;  // n_tris words
    const uint32_t *inv_perm;   // non-null: stored row = inv_perm[prim] (the caller's numbering after a build form); a word >= n_tris makes the record invalid
    uint32_t n_tris;
};

// out[4 * perm[s] + q] = tris[4 * s + q] for the n stored rows on `stream`: the rows in update order.  `out` holds n rows, 16-byte aligned.
hipError_t surface_scatter_rows(hipStream_t stream, const float4 *tris, const uint32_t *perm, uint32_t n, void *out);
// Answers records[0 .. n) in place on `stream`: one record per lane, the second and third float4 of a record are written.
hipError_t surface_launch(hipStream_t stream, const SurfaceScene &scene, void *records, uint32_t n);

}  // namespace rv
