// sevenzenc_kernels.hip -- the pack stage of the 7z writer for gfx950: the
// phases of sevenz_pack_device.h as four launches on one stream.
//
//   szpack_collect_kernel   a tile of 256 pieces per workgroup: values, the
//                           first failed piece (atomicMin, only failed pieces
//                           touch it), the tile's sum
//   szpack_tiles_kernel     one workgroup: the tile sums become tile bases, the
//                           total and the verdict.  2^20 pieces are 4,096 tile
//                           sums, 16 per thread
//   szpack_offsets_kernel   per tile: piece offsets and folder starts
//   szpack_gather_kernel    one workgroup per piece (a grid-stride loop above
//                           2^20 pieces): the 16-byte-vector move, the 0x00
//                           after an LZMA2 folder, the folder's pack size
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "sevenz_pack_device.h"
#include "sevenzenc_internal.h"

namespace {

using szpack::kThreads;

__global__ void __launch_bounds__(kThreads) szpack_collect_kernel(SzGpuPackArgs a) {
  __shared__ uint64_t sh[kThreads];
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(szpack::bad_of(a));
  sh[threadIdx.x] = szpack::collect_item(a, i, [bad](uint64_t k) { atomicMin(bad, k); });
  __syncthreads();
  if (threadIdx.x == 0) szpack::collect_tile(a, blockIdx.x, sh);
}

__global__ void __launch_bounds__(kThreads) szpack_tiles_kernel(SzGpuPackArgs a) {
  __shared__ uint64_t part[kThreads];
  part[threadIdx.x] = szpack::tiles_part(a, threadIdx.x);
  __syncthreads();
  if (threadIdx.x == 0) szpack::tiles_total(a, part);
  __syncthreads();
  szpack::tiles_write(a, threadIdx.x, part[threadIdx.x]);
}

__global__ void __launch_bounds__(kThreads) szpack_offsets_kernel(SzGpuPackArgs a) {
  __shared__ uint64_t sh[kThreads];
  const uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
  sh[threadIdx.x] = i < a.n ? szpack::values_of(a)[i] : 0;
  __syncthreads();
  if (threadIdx.x == 0) szpack::offsets_tile(a, blockIdx.x, sh);
  __syncthreads();
  szpack::offsets_item(a, i, sh[threadIdx.x]);
}

__global__ void __launch_bounds__(kThreads) szpack_gather_kernel(SzGpuPackArgs a) {
  if (a.d_total->res != szpack::kOk) return;  // nothing is written
  for (uint64_t i = blockIdx.x; i < a.n; i += gridDim.x) szpack::gather_thread(a, i, threadIdx.x);
}

}  // namespace

extern "C" int szpackgpu_launch(const SzGpuPackArgs* args, hipStream_t stream) {
  const SzGpuPackArgs a = *args;
  const uint64_t tiles = szpack::tiles_of(a.n);
  if (a.n > 0x7FFFFFFFull) return -2;
  if (hipMemsetAsync(szpack::bad_of(a), 0xFF, sizeof(uint64_t), stream) != hipSuccess) return -1;
  if (tiles) {
    hipLaunchKernelGGL(szpack_collect_kernel, dim3(uint32_t(tiles)), dim3(kThreads), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  hipLaunchKernelGGL(szpack_tiles_kernel, dim3(1), dim3(kThreads), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -1;
  if (tiles == 0) return 0;
  hipLaunchKernelGGL(szpack_offsets_kernel, dim3(uint32_t(tiles)), dim3(kThreads), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -1;
  const uint32_t grid = uint32_t(a.n < (1u << 20) ? a.n : (1u << 20));
  hipLaunchKernelGGL(szpack_gather_kernel, dim3(grid), dim3(kThreads), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
