// lzmaenc_normal_kernels.hip -- the LZMA normal-mode encode kernel for gfx950
// (the optimal parser and / or the Bt4 finder: lzmaenc_device.h's
// LzmaEncNormal), in a translation unit of its own because its encoder is
// built differently from the fast path's.
//
// LZENC_DEVICE_NOINLINE makes ReadMatchDistances a real call, which keeps the
// encoder's state in scratch memory (272 bytes per lane) instead of registers.
// An open defect stands behind it.  With every function forced inline at -O3,
// as lzmaenc_kernels.hip builds the fast path, this kernel (220 VGPRs, no
// scratch) encoded some streams to valid LZMA of the reference's length or one
// byte more, but not to the reference's bytes: the same wrong bytes on every
// run, whatever the workspace held, in each of the three normal modes.  The
// same source gives the reference's bytes on the host (g++ -O2, clang++ -O3,
// ASan, UBSan and MSan builds), on the device at -O1, and on the device at -O3
// as soon as any one of these is a real call: get_matches and skip,
// read_match_distances, code_block, get_optimum and get_optimum_fast, or the
// Bt4 functions -- five builds, each right on the streams that had gone wrong.
// So no one function's inlining is at fault; what the wrong build has that
// the others lack is the whole state in registers.  The cause was not found.
// tests/test_lzmaenc_opt_gpu.py compares every stream with the reference, so a
// build that goes wrong again fails there; DESIGN.md states the defect.
#define LZENC_DEVICE_NOINLINE 1
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "lzmaenc_device.h"
#include "lzmaenc_internal.h"

namespace {

// lzmaenc_encode_kernel's geometry: one wave per workgroup, `lanes` streams per
// wave, ProbPrices (512 bytes) in LDS beside the CRC table.  It walks the same
// order and leaves mode-0 and rejected streams to the fast kernel; a workgroup
// without a stream of its own returns before it builds the tables.
__global__ void __launch_bounds__(64) lzmaenc_encode_normal_kernel(
    const LzmaEncGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order, uint32_t n,
    uint32_t lanes, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
    uint8_t* __restrict__ ws, LzmaEncGpuResult* __restrict__ results) {
  __shared__ uint32_t crc[256];
  __shared__ uint32_t prob_prices[lzenc::kProbPricesWords];
  const uint64_t k = uint64_t(blockIdx.x) * lanes + threadIdx.x;
  uint32_t id = 0;
  bool mine = threadIdx.x < lanes && k < n;
  if (mine) {
    id = order ? order[k] : uint32_t(k);
    mine = id < n;
  }
  LzmaEncGpuStreamDesc d;
  if (mine) {
    d = descs[id];
    mine = d.mode != 0 && lzmaenc_check(d) == lzenc::kOk;
  }
  if (!__syncthreads_or(mine)) return;
  for (uint32_t v = threadIdx.x; v < 256; v += 64) crc[v] = lzenc::crc_entry(v);
  for (uint32_t v = threadIdx.x; v < lzenc::kProbPricesWords; v += 64)
    prob_prices[v] = lzenc::prob_price_entry(v);
  __syncthreads();
  if (!mine) return;
  const lzenc::Params q = lzmaenc_params(d);
  const lzenc::Layout l = lzenc::lzmaenc_layout(q, d.src_len);
  lzenc::LzmaEncNormal e;
  const lzenc::Out o = e.encode(src + d.src_off, uint32_t(d.src_len), dst + d.dst_off, d.dst_cap,
                                q, ws + d.ws_off, l, crc, prob_prices);
  LzmaEncGpuResult r;
  r.res = o.res;
  r._pad = 0;
  r.dest_len = o.dest_len;
  results[id] = r;
}

}  // namespace

extern "C" int lzmaencgpu_launch_normal(const LzmaEncGpuStreamDesc* d_descs,
                                        const uint32_t* d_order, uint32_t n, const uint8_t* d_src,
                                        uint8_t* d_dst, uint8_t* d_ws, LzmaEncGpuResult* d_results,
                                        uint32_t lanes, hipStream_t stream) {
  const uint32_t groups = uint32_t((uint64_t(n) + lanes - 1) / lanes);
  hipLaunchKernelGGL(lzmaenc_encode_normal_kernel, dim3(groups), dim3(64), 0, stream, d_descs,
                     d_order, n, lanes, d_src, d_dst, d_ws, d_results);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
