// bcj2enc_kernels.hip -- the BCJ2 encoder for gfx950: the phases of
// bcj2enc_device.h as five launches on one stream.
//
//   bcj2enc_plan_kernel      one workgroup: the streams' first segments and
//                            scratch slices, the batch's segment count
//   bcj2enc_classify_kernel  a wave per 1 KiB segment, four segments per
//                            workgroup step, a grid-stride loop over the
//                            batch's segments (the count lives on the device,
//                            so the grid is a fixed 8 workgroups per CU and
//                            every wave of a workgroup runs the same number of
//                            steps: the barriers of the scan are uniform)
//   bcj2enc_streams_kernel   one wave per stream, 64 segments per step
//   bcj2enc_scatter_kernel   as classify, then the forward walk of each run
//   bcj2enc_code_kernel      one lane per stream, the 258 cells in the lane's
//                            LDS slice (as the decoder's kernel has them)
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "bcj2enc_device.h"
#include "bcj2enc_internal.h"
#include "lzma_gpu_internal.h"

namespace {

using namespace bcj2enc;
typedef lzgpu::bcj2_gbyte gb;

__global__ void __launch_bounds__(kThreads) bcj2enc_plan_kernel(Args a) {
  __shared__ uint64_t segs[kThreads], bytes[kThreads];
  plan_part(a, threadIdx.x, &segs[threadIdx.x], &bytes[threadIdx.x]);
  __syncthreads();
  if (threadIdx.x == 0) plan_total(a, segs, bytes);
  __syncthreads();
  plan_write(a, threadIdx.x, segs[threadIdx.x], bytes[threadIdx.x]);
}

// the inclusive scan of the wave's elements: buf[0] holds them, the result is
// in buf[kScanOut]; every wave of the workgroup calls it together
__device__ __forceinline__ void wave_scan(Elem (*buf)[kWave], uint32_t lane) {
#pragma unroll
  for (uint32_t k = 0; k < kScanSteps; ++k) {
    __syncthreads();
    scan_step(buf[k & 1], buf[(k + 1) & 1], lane, k);
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kThreads) bcj2enc_classify_kernel(Args a) {
  __shared__ Elem sh[kWaves][2][kWave];
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const uint64_t total = header_of(a)->segs;
  for (uint64_t first = uint64_t(blockIdx.x) * kWaves; first < total;
       first += uint64_t(gridDim.x) * kWaves) {
    const SegRef r = seg_ref(a, first + wave);
    sh[wave][0][lane] = seg_elem(a, r, lane, (const gb*)a.src);
    wave_scan(sh[wave], lane);
    if (lane == kWave - 1) classify_put(a, r, sh[wave][kScanOut][lane]);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kThreads) bcj2enc_scatter_kernel(Args a) {
  __shared__ Elem sh[kWaves][2][kWave];
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const uint64_t total = header_of(a)->segs;
  for (uint64_t first = uint64_t(blockIdx.x) * kWaves; first < total;
       first += uint64_t(gridDim.x) * kWaves) {
    const SegRef r = seg_ref(a, first + wave);
    sh[wave][0][lane] = seg_elem(a, r, lane, (const gb*)a.src);
    wave_scan(sh[wave], lane);
    scatter_thread(a, r, lane, sh[wave][kScanOut], (const gb*)a.src, (gb*)a.dst);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kWave) bcj2enc_streams_kernel(Args a) {
  __shared__ Elem maps[2][kWave], sums[2][kWave];
  const uint64_t stream = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const uint64_t segs = segs_of(a.descs[stream].src_len);
  uint32_t carry = 0, tot[3] = {0, 0, 0};
  for (uint64_t first = 0; first < segs; first += kWave) {
    maps[0][lane] = streams_map(a, stream, first, lane);
    wave_scan(maps, lane);
    const Elem own = streams_counts(a, stream, first, lane, maps[kScanOut], carry);
    sums[0][lane] = own;
#pragma unroll
    for (uint32_t k = 0; k < kScanSteps; ++k) {
      __syncthreads();
      add_step(sums[k & 1], sums[(k + 1) & 1], lane, k);
    }
    __syncthreads();
    streams_put(a, stream, first, lane, own, sums[kScanOut], tot);
    streams_next(maps[kScanOut], sums[kScanOut], &carry, tot);
    __syncthreads();
  }
  if (lane == 0) streams_total(a, stream, tot);
}

__global__ void __launch_bounds__(kWave) bcj2enc_code_kernel(Args a) {
  __shared__ uint16_t probs[kWave * 258];
  const uint64_t stream = uint64_t(blockIdx.x) * kWave + threadIdx.x;
  if (stream >= a.n) return;
  typedef __attribute__((address_space(3))) uint16_t lds16;
  code_stream(a, stream, (gb*)a.dst, (lds16*)probs + threadIdx.x * 258);
}

}  // namespace

extern "C" int bcj2encgpu_launch(const Bcj2GpuEncDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                 uint8_t* d_dst, uint8_t* d_scratch, Bcj2GpuEncResult* d_results,
                                 unsigned phases, hipStream_t stream) {
  if (n == 0) return 0;
  Args a;
  a.descs = d_descs;
  a.n = n;
  a.src = d_src;
  a.dst = d_dst;
  a.scratch = d_scratch;
  a.results = d_results;
  const uint32_t grid = lzgpu_host::device_cus() * 8;
  if (phases & kBcj2EncSplit) {
    hipLaunchKernelGGL(bcj2enc_plan_kernel, dim3(1), dim3(kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(bcj2enc_classify_kernel, dim3(grid), dim3(kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(bcj2enc_streams_kernel, dim3(n), dim3(kWave), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(bcj2enc_scatter_kernel, dim3(grid), dim3(kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  if (!(phases & kBcj2EncCode)) return 0;
  hipLaunchKernelGGL(bcj2enc_code_kernel, dim3((n + kWave - 1) / kWave), dim3(kWave), 0, stream,
                     a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
