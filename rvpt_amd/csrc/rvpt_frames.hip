// rvpt_frames.hip — frames that stay on the device: the layout kernels of rvpt_hip_read / rvpt_hip_write_accum for device memory that is only 4-byte aligned (a
// view into a larger tensor).  read_rowmajor and tile_rgba32f (rvpt_kernels.hip) move a pixel as one float4, which needs 16-byte alignment on the row-major
// side; these move the same values float by float, one thread per float, so that neighbouring lanes still touch neighbouring dwords on both sides.  Pure
// copies: no arithmetic, hence the same bytes.  Not frame kernels: this file is outside build.py's KERNEL_SOURCES, so kernel_sha and the profiles stamped with it stand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rvpt_frames.h"
#include "rvpt_kernels.h"

namespace rv {

__global__ void read_rowmajor_dwords(const float *__restrict__ accum, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tile_rank, uint32_t tile_world,
                                     float *__restrict__ dst)
{
    const uint32_t xf = blockIdx.x * blockDim.x + threadIdx.x;  // float of the row: pixel xf / 4, component xf % 4
    const uint32_t y = blockIdx.y * blockDim.y + threadIdx.y;
    const uint32_t x = xf >> 2;
    if (x >= width || y >= height) return;
    const uint32_t tile = tile_slot(x >> 4, y >> 4, tiles_x);
    float v = 0.f;
    if (tile % tile_world == tile_rank) v = accum[(static_cast<size_t>(tile / tile_world) * 256u + ((y & 15u) << 4) + (x & 15u)) * 4u + (xf & 3u)];
    dst[(static_cast<size_t>(y) * width + x) * 4u + (xf & 3u)] = v;
}

__global__ void tile_rgba32f_dwords(const float *__restrict__ src, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tile_rank, uint32_t tile_world,
                                    uint32_t n_work, float *__restrict__ accum)
{
    const size_t f = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // float of the accumulator
    const uint32_t work = static_cast<uint32_t>(f >> 2);
    if (f >= static_cast<size_t>(n_work) * 4u) return;
    uint32_t tx, ty;
    slot_tile((work >> 8) * tile_world + tile_rank, tiles_x, tx, ty);
    const uint32_t gx = tx * 16u + (work & 15u), gy = ty * 16u + ((work & 255u) >> 4);
    float v = 0.f;
    if (gx < width && gy < height) v = src[(static_cast<size_t>(gy) * width + gx) * 4u + (f & 3u)];
    accum[f] = v;
}

}  // namespace rv
