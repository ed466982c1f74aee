// lzma86_kernels.hip -- the kernels of the Lzma86 batch for gfx950: thin
// wrappers over lzma86_device.h (one call per thread).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "lzma86_device.h"
#include "lzma86_internal.h"

using namespace lz86;

// blockIdx.x walks the jobs, blockIdx.y is the workgroup's share of a job
__global__ void __launch_bounds__(kThreads) lzma86_stage_kernel(
    const StageJob* __restrict__ jobs, uint32_t n, const uint8_t* __restrict__ src_base,
    uint8_t* __restrict__ filt_base) {
  for (uint32_t j = blockIdx.x; j < n; j += gridDim.x)
    stage_thread(jobs, j, src_base, filt_base, threadIdx.x, blockIdx.y, gridDim.y);
}

// one wave per stream, four streams per workgroup
__global__ void __launch_bounds__(kThreads) lzma86_select_kernel(
    const Stream* __restrict__ streams, uint32_t n, const LzmaEncGpuResult* __restrict__ cand,
    const uint8_t* __restrict__ slots, uint8_t* __restrict__ dst,
    Lzma86GpuResult* __restrict__ results, uint64_t split) {
  const uint32_t waves = kThreads / kWave;
  const uint32_t w = threadIdx.x / kWave, t = threadIdx.x % kWave;
  for (uint64_t i = uint64_t(blockIdx.x) * waves + w; i < n; i += uint64_t(gridDim.x) * waves)
    select_thread(streams, i, cand, slots, dst, results, split, t);
}

__global__ void __launch_bounds__(kThreads) lzma86_gather_kernel(
    const Stream* __restrict__ streams, const uint32_t* __restrict__ large, uint32_t n_large,
    const LzmaEncGpuResult* __restrict__ cand, const uint8_t* __restrict__ slots,
    uint8_t* __restrict__ dst, uint64_t split) {
  for (uint32_t k = blockIdx.x; k < n_large; k += gridDim.x)
    gather_thread(streams, large[k], cand, slots, dst, split, threadIdx.x, blockIdx.y, gridDim.y);
}

__global__ void __launch_bounds__(kThreads) lzma86_finish_kernel(
    const DecStream* __restrict__ streams, uint32_t n, const LzmaGpuResult* __restrict__ lzma,
    Lzma86GpuResult* __restrict__ results, uint64_t* __restrict__ x86_len) {
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (i < n) finish_thread(streams, i, lzma, results, x86_len);
}

uint64_t lzma86_split() {
  const char* v = getenv("LZGPU_LZMA86_SPLIT");
  return v ? strtoull(v, nullptr, 10) : kLzma86SplitDefault;
}

static uint32_t grid_y(uint32_t parts) {
  return parts == 0 ? 1u : (parts > kLzma86PartsMax ? kLzma86PartsMax : parts);
}
// the kernels stride over their items in x: at most 2^20 workgroups in all
static uint32_t grid_x(uint32_t n, uint32_t gy) {
  const uint32_t most = (1u << 20) / gy;
  return n < most ? n : most;
}

extern "C" int lzma86gpu_launch_stage(const StageJob* d_jobs, uint32_t n, uint32_t parts,
                                      const uint8_t* src_base, uint8_t* filt_base,
                                      hipStream_t stream) {
  if (n == 0) return 0;
  const uint32_t gy = grid_y(parts);
  hipLaunchKernelGGL(lzma86_stage_kernel, dim3(grid_x(n, gy), gy), dim3(kThreads), 0, stream,
                     d_jobs, n, src_base, filt_base);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzma86gpu_launch_select(const Stream* d_streams, uint32_t n,
                                       const LzmaEncGpuResult* d_cand, const uint8_t* d_slots,
                                       uint8_t* d_dst, Lzma86GpuResult* d_results,
                                       const uint32_t* d_large, uint32_t n_large, uint32_t parts,
                                       uint64_t split, hipStream_t stream) {
  if (n == 0) return 0;
  const uint32_t waves = kThreads / kWave;
  const uint32_t groups = (n + waves - 1) / waves;
  hipLaunchKernelGGL(lzma86_select_kernel, dim3(groups < 65536 ? groups : 65536), dim3(kThreads),
                     0, stream, d_streams, n, d_cand, d_slots, d_dst, d_results, split);
  if (hipGetLastError() != hipSuccess) return -1;
  if (n_large == 0) return 0;
  const uint32_t gy = grid_y(parts);
  hipLaunchKernelGGL(lzma86_gather_kernel, dim3(grid_x(n_large, gy), gy), dim3(kThreads), 0,
                     stream, d_streams, d_large, n_large, d_cand, d_slots, d_dst, split);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzma86gpu_launch_finish(const DecStream* d_streams, uint32_t n,
                                       const LzmaGpuResult* d_lzma, Lzma86GpuResult* d_results,
                                       uint64_t* d_x86_len, hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(lzma86_finish_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     stream, d_streams, n, d_lzma, d_results, d_x86_len);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
