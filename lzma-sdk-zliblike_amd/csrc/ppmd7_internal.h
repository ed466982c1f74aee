// ppmd7_internal.h -- the PPMd7 workspace slice layout and launcher, shared by
// ppmd7_kernels.hip, ppmd7enc_kernels.hip, ppmd7_capi.hip and sevenz_capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lzma_gpu.h"

// A stream's slice: the model (alignment offset + mem_size + the 12-byte list
// head), padded to 256 bytes, then
// BinSumm (128 x 64 16-bit cells).
__host__ __device__ inline uint64_t ppmd7_bin_offset(uint32_t mem_size) {
  const uint64_t model = uint64_t(4u - (mem_size & 3u)) + mem_size + 12u;
  return (model + 255u) & ~uint64_t(255);
}
__host__ __device__ inline uint64_t ppmd7_slice_bytes(uint32_t mem_size) {
  return ppmd7_bin_offset(mem_size) + 128u * 64u * 2u;
}

// one workgroup per stream.  0 on success.
extern "C" int ppmd7gpu_launch(const Ppmd7GpuStreamDesc* d_descs, uint32_t n, const uint8_t* d_src,
                               uint8_t* d_dst, uint8_t* d_ws, Ppmd7GpuResult* d_results,
                               hipStream_t stream);
// the encoder (ppmd7enc_kernels.hip): the same shape and slices
extern "C" int ppmd7encgpu_launch(const Ppmd7GpuEncDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                  uint8_t* d_dst, uint8_t* d_ws, Ppmd7GpuEncResult* d_results,
                                  hipStream_t stream);
