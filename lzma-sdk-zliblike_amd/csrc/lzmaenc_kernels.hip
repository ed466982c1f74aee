// lzmaenc_kernels.hip -- LZMA batch encoding for gfx950: one stream
// per lane, lzmaenc_device.h's encoder with its range-coder and parser state in
// registers and its tables (probability cells, `matches`, hash, `son` ring) in
// the stream's workspace slice.  The work is pointer chasing through the hash
// chains, and nothing is wave-uniform: the waves' job is to keep many chains in
// flight.
//
//   lzmaenc_init_kernel    the whole grid clears the hashes (516 KiB per stream
//                          at the smallest dictionary) and sets the probability
//                          cells; the encoding lane never does
//   lzmaenc_encode_kernel  one wave per workgroup, `lanes` streams per wave (the
//                          other lanes leave at once).  The match finder's CRC
//                          table (1 KiB) is built in LDS before the loop; the
//                          encode loop has no block-wide synchronisation, and a
//                          lane whose stream is rejected, empty or finished just
//                          returns.  Mode 0 (the fast path) only: a lane whose
//                          stream has a normal mode returns before it touches
//                          memory.
//   lzmaenc_encode_normal_kernel  (lzmaenc_normal_kernels.hip) the same geometry for the normal modes (the
//                          optimal parser and / or Bt4: LzmaEncNormal), with
//                          ProbPrices (512 bytes) in LDS beside the CRC table.
//                          It walks the same order and leaves mode-0 and
//                          rejected streams to the kernel above; a workgroup
//                          without a stream of its own returns before it builds
//                          the tables.
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "lzmaenc_device.h"
#include "lzmaenc_internal.h"

namespace {

constexpr uint32_t kInitThreads = 256;

// (stream, part) pairs dealt over the grid: part p of `parts` takes cells and
// hash words p * 256 + thread, stepping by parts * 256
__global__ void __launch_bounds__(kInitThreads) lzmaenc_init_kernel(
    const LzmaEncGpuStreamDesc* __restrict__ descs, uint32_t n, uint32_t parts,
    uint8_t* __restrict__ ws) {
  const uint64_t total = uint64_t(n) * parts;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint32_t s = uint32_t(w / parts), part = uint32_t(w % parts);
    const LzmaEncGpuStreamDesc d = descs[s];
    if (lzmaenc_check(d) != lzenc::kOk) continue;
    const lzenc::Layout l = lzenc::lzmaenc_layout(lzmaenc_params(d), d.src_len);
    lzenc::lzmaenc_init_slice(ws + d.ws_off, l, uint64_t(part) * kInitThreads + threadIdx.x,
                              uint64_t(parts) * kInitThreads);
  }
}

__global__ void __launch_bounds__(64) lzmaenc_encode_kernel(
    const LzmaEncGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order, uint32_t n,
    uint32_t lanes, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
    uint8_t* __restrict__ ws, LzmaEncGpuResult* __restrict__ results) {
  __shared__ uint32_t crc[256];
  for (uint32_t v = threadIdx.x; v < 256; v += 64) crc[v] = lzenc::crc_entry(v);
  __syncthreads();
  if (threadIdx.x >= lanes) return;
  const uint64_t k = uint64_t(blockIdx.x) * lanes + threadIdx.x;
  if (k >= n) return;
  const uint32_t id = order ? order[k] : uint32_t(k);
  if (id >= n) return;
  const LzmaEncGpuStreamDesc d = descs[id];
  lzenc::Out o;
  o.res = lzmaenc_check(d);
  o.dest_len = 0;
  if (o.res == lzenc::kOk && d.mode != 0) return;  // lzmaenc_encode_normal_kernel's
  if (o.res == lzenc::kOk) {
    const lzenc::Params q = lzmaenc_params(d);
    const lzenc::Layout l = lzenc::lzmaenc_layout(q, d.src_len);
    lzenc::LzmaEnc e;
    o = e.encode(src + d.src_off, uint32_t(d.src_len), dst + d.dst_off, d.dst_cap, q,
                 ws + d.ws_off, l, crc);
  }
  LzmaEncGpuResult r;
  r.res = o.res;
  r._pad = 0;
  r.dest_len = o.dest_len;
  results[id] = r;
}

}  // namespace

extern "C" int lzmaencgpu_launch_init(const LzmaEncGpuStreamDesc* d_descs, uint32_t n,
                                      uint8_t* d_ws, hipStream_t stream) {
  if (n == 0) return 0;
  // at least ~4,096 workgroups of 256 for the clear, at most 64 parts a stream
  uint32_t parts = (4096 + n - 1) / n;
  if (parts > 64) parts = 64;
  if (parts < 1) parts = 1;
  const uint64_t want = uint64_t(n) * parts;
  const uint32_t grid = uint32_t(want < 65536 ? want : 65536);
  hipLaunchKernelGGL(lzmaenc_init_kernel, dim3(grid), dim3(kInitThreads), 0, stream, d_descs, n,
                     parts, d_ws);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzmaencgpu_launch(const LzmaEncGpuStreamDesc* d_descs, const uint32_t* d_order,
                                 uint32_t n, const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_ws,
                                 LzmaEncGpuResult* d_results, uint32_t lanes, hipStream_t stream,
                                 uint32_t kernels) {
  if (n == 0) return 0;
  if (lanes != 0 && lanes != 16 && lanes != 32 && lanes != 64) return -2;
  if (lzmaencgpu_launch_init(d_descs, n, d_ws, stream) != 0) return -1;
  // the normal modes first: they come first in the order and take longest
  if ((kernels & kLzmaEncKernelNormal) &&
      lzmaencgpu_launch_normal(d_descs, d_order, n, d_src, d_dst, d_ws, d_results,
                               lanes ? lanes : kLzmaEncLanesNormalDefault, stream) != 0)
    return -1;
  if (kernels & kLzmaEncKernelFast) {
    const uint32_t lf = lanes ? lanes : kLzmaEncLanesDefault;
    const uint32_t groups = uint32_t((uint64_t(n) + lf - 1) / lf);
    hipLaunchKernelGGL(lzmaenc_encode_kernel, dim3(groups), dim3(64), 0, stream, d_descs, d_order,
                       n, lf, d_src, d_dst, d_ws, d_results);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}
