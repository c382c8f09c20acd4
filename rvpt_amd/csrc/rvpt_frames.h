// rvpt_frames.h — the kernels of frames that stay on the device (rvpt_frames.hip): rvpt_hip_read into, and rvpt_hip_write_accum from, device memory that is
// only 4-byte aligned (rvpt_abi.hip).  A 16-byte aligned device pointer rides the kernels the host route has (rvpt_kernels.h: read_rowmajor, tile_rgba32f).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rv {

// this rank's tiles -> row-major RGBA32F, one thread per FLOAT (x counts floats: 4 per pixel); pixels of foreign tiles become 0.  read_rowmajor's values, 4-byte stores
__global__ void read_rowmajor_dwords(const float *__restrict__ accum, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tile_rank, uint32_t tile_world,
                                     float *__restrict__ dst);
// row-major RGBA32F -> this rank's tile-linear accumulator, one thread per FLOAT of it (n_work pixels); tile_rgba32f's values, 4-byte loads
__global__ void tile_rgba32f_dwords(const float *__restrict__ src, uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t tile_rank, uint32_t tile_world,
                                    uint32_t n_work, float *__restrict__ accum);

}  // namespace rv
