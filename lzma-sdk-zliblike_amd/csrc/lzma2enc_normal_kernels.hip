// lzma2enc_normal_kernels.hip -- the LZMA2 normal-mode block encode kernel for
// gfx950 (lzma2enc_device.h's Lzma2EncNormal), built out of line for the reason
// lzmaenc_normal_kernels.hip gives.
#define LZENC_DEVICE_NOINLINE 1
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "lzma2enc_device.h"
#include "lzma2enc_internal.h"

namespace {

// lzma2enc_encode_kernel's geometry with ProbPrices in LDS beside the CRC
// table; it walks the same order and leaves mode-0 and rejected blocks to the
// fast kernel.
__global__ void __launch_bounds__(64) lzma2enc_encode_normal_kernel(
    const LzmaEncGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order,
    uint32_t first, uint32_t count, uint32_t n, uint32_t lanes, const uint8_t* __restrict__ src,
    uint8_t* __restrict__ dst, uint8_t* __restrict__ ws, LzmaEncGpuResult* __restrict__ results) {
  __shared__ uint32_t crc[256];
  __shared__ uint32_t prob_prices[lzenc::kProbPricesWords];
  const uint64_t k = uint64_t(blockIdx.x) * lanes + threadIdx.x;
  uint32_t id = 0;
  bool mine = threadIdx.x < lanes && k < count;
  if (mine) {
    id = order ? order[first + k] : uint32_t(first + k);
    mine = id < n;
  }
  LzmaEncGpuStreamDesc d;
  if (mine) {
    d = descs[id];
    mine = d.mode != 0 && lzma2enc_check(d) == lzenc::kOk;
  }
  if (!__syncthreads_or(mine)) return;
  for (uint32_t v = threadIdx.x; v < 256; v += 64) crc[v] = lzenc::crc_entry(v);
  for (uint32_t v = threadIdx.x; v < lzenc::kProbPricesWords; v += 64)
    prob_prices[v] = lzenc::prob_price_entry(v);
  __syncthreads();
  if (!mine) return;
  const lzenc::Params q = lzmaenc_params(d);
  const lzenc::Layout2 m = lzenc::lzma2enc_layout(q, d.src_len);
  lzenc::Lzma2EncNormal e;
  const lzenc::Out o = e.encode_block(src + d.src_off, uint32_t(d.src_len), dst + d.dst_off,
                                      d.dst_cap, q, ws + d.ws_off, m, crc, prob_prices);
  LzmaEncGpuResult r;
  r.res = o.res;
  r._pad = 0;
  r.dest_len = o.dest_len;
  results[id] = r;
}

}  // namespace

extern "C" int lzma2encgpu_launch_normal(const LzmaEncGpuStreamDesc* d_descs,
                                         const uint32_t* d_order, uint32_t first, uint32_t count,
                                         uint32_t n, const uint8_t* d_src, uint8_t* d_dst,
                                         uint8_t* d_ws, LzmaEncGpuResult* d_results,
                                         uint32_t lanes, hipStream_t stream) {
  const uint32_t groups = uint32_t((uint64_t(count) + lanes - 1) / lanes);
  hipLaunchKernelGGL(lzma2enc_encode_normal_kernel, dim3(groups), dim3(64), 0, stream, d_descs,
                     d_order, first, count, n, lanes, d_src, d_dst, d_ws, d_results);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
