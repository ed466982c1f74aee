// lzma2enc_kernels.hip -- LZMA2 block encoding for gfx950: one block
// per lane (lzma2enc_device.h's chunk driver over lzmaenc_device.h's encoder),
// and the compaction that turns the blocks' slots into one LZMA2 stream
// without a visit to the host.
//
//   lzma2enc_init_kernel     lzmaenc_init_kernel's pattern over the LZMA2
//                            layout: the whole grid clears the hashes and sets
//                            the probability cells; the saved table needs none
//                            (it is written before it is read)
//   lzma2enc_encode_kernel   lzmaenc_encode_kernel's geometry: one wave per
//                            workgroup, `lanes` blocks per wave, the CRC table
//                            in LDS, no synchronisation in the loop; mode 0
//                            (the fast path) only
//   lzma2enc_encode_normal_kernel  (lzma2enc_normal_kernels.hip) the same for the normal modes (the optimal
//                            parser and / or Bt4: Lzma2EncNormal), ProbPrices
//                            in LDS beside the CRC table; it walks the same
//                            order and leaves mode-0 and rejected blocks to the
//                            kernel above
//   lzma2enc_scan_kernel     one workgroup: exclusive scan of the blocks'
//                            dest_len, the first failed block, the total
//   lzma2enc_compact_kernel  one workgroup per block gathers its bytes from its
//                            slot to its place in the stream; block 0 adds the
//                            final 0x00.  Source and destination are
//                            byte-aligned only: the body moves as 16-byte
//                            stores aligned to the destination, each made from
//                            two aligned 16-byte loads, head and tail by bytes
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "lzma2enc_device.h"
#include "lzma2enc_internal.h"

namespace {

constexpr uint32_t kInitThreads = 256;
constexpr uint32_t kMoveThreads = 256;

__global__ void __launch_bounds__(kInitThreads) lzma2enc_init_kernel(
    const LzmaEncGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order,
    uint32_t first, uint32_t count, uint32_t n, uint32_t parts, uint8_t* __restrict__ ws) {
  const uint64_t total = uint64_t(count) * parts;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint32_t k = first + uint32_t(w / parts), part = uint32_t(w % parts);
    const uint32_t id = order ? order[k] : k;
    if (id >= n) continue;
    const LzmaEncGpuStreamDesc d = descs[id];
    if (lzma2enc_check(d) != lzenc::kOk) continue;
    const lzenc::Layout2 m = lzenc::lzma2enc_layout(lzmaenc_params(d), d.src_len);
    lzenc::lzmaenc_init_slice(ws + d.ws_off, m.l, uint64_t(part) * kInitThreads + threadIdx.x,
                              uint64_t(parts) * kInitThreads);
  }
}

__global__ void __launch_bounds__(64) lzma2enc_encode_kernel(
    const LzmaEncGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order,
    uint32_t first, uint32_t count, uint32_t n, uint32_t lanes, const uint8_t* __restrict__ src,
    uint8_t* __restrict__ dst, uint8_t* __restrict__ ws, LzmaEncGpuResult* __restrict__ results) {
  __shared__ uint32_t crc[256];
  for (uint32_t v = threadIdx.x; v < 256; v += 64) crc[v] = lzenc::crc_entry(v);
  __syncthreads();
  if (threadIdx.x >= lanes) return;
  const uint64_t k = uint64_t(blockIdx.x) * lanes + threadIdx.x;
  if (k >= count) return;
  const uint32_t id = order ? order[first + k] : uint32_t(first + k);
  if (id >= n) return;
  const LzmaEncGpuStreamDesc d = descs[id];
  lzenc::Out o;
  o.res = lzma2enc_check(d);
  o.dest_len = 0;
  if (o.res == lzenc::kOk && d.mode != 0) return;  // lzma2enc_encode_normal_kernel's
  if (o.res == lzenc::kOk) {
    const lzenc::Params q = lzmaenc_params(d);
    const lzenc::Layout2 m = lzenc::lzma2enc_layout(q, d.src_len);
    lzenc::Lzma2Enc e;
    o = e.encode_block(src + d.src_off, uint32_t(d.src_len), dst + d.dst_off, d.dst_cap, q,
                       ws + d.ws_off, m, crc);
  }
  LzmaEncGpuResult r;
  r.res = o.res;
  r._pad = 0;
  r.dest_len = o.dest_len;
  results[id] = r;
}

// offsets[i] = sum of dest_len[0, i), offsets[n] = the sum; total->dest_len =
// the sum + 1 (the final 0x00).  total->res: the first failed block's res
// (_pad = its index), else SZ_ERROR_OUTPUT_EOF when the stream does not fit
// out_cap, else SZ_OK.
__global__ void __launch_bounds__(kMoveThreads) lzma2enc_scan_kernel(
    const LzmaEncGpuResult* __restrict__ results, uint32_t n, uint64_t out_cap,
    uint64_t* __restrict__ offsets, LzmaEncGpuResult* __restrict__ total) {
  __shared__ uint64_t part[kMoveThreads];
  __shared__ uint32_t bad;
  const uint32_t t = threadIdx.x;
  if (t == 0) bad = 0xFFFFFFFFu;
  __syncthreads();
  const uint32_t per = (n + kMoveThreads - 1) / kMoveThreads;
  const uint64_t lo = uint64_t(t) * per;
  const uint64_t hi = lo + per < n ? lo + per : n;
  uint64_t sum = 0;
  for (uint64_t i = lo; i < hi; ++i) {
    sum += results[i].dest_len;
    if (results[i].res != lzenc::kOk) atomicMin(&bad, uint32_t(i));
  }
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint64_t run = 0;
    for (uint32_t j = 0; j < kMoveThreads; ++j) {
      const uint64_t v = part[j];
      part[j] = run;
      run += v;
    }
    offsets[n] = run;
    LzmaEncGpuResult r;
    r.res = bad != 0xFFFFFFFFu ? results[bad].res
                               : (run + 1 > out_cap ? lzenc::kErrOutputEof : lzenc::kOk);
    r._pad = bad != 0xFFFFFFFFu ? bad : 0;
    r.dest_len = run + 1;
    *total = r;
  }
  __syncthreads();
  uint64_t at = part[t];
  for (uint64_t i = lo; i < hi; ++i) {
    offsets[i] = at;
    at += results[i].dest_len;
  }
}

__device__ __forceinline__ uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t bits) {
  return uint32_t(((uint64_t(hi) << 32) | lo) >> bits);
}

__global__ void __launch_bounds__(kMoveThreads) lzma2enc_compact_kernel(
    const LzmaEncGpuStreamDesc* __restrict__ descs, const LzmaEncGpuResult* __restrict__ results,
    const uint64_t* __restrict__ offsets, const LzmaEncGpuResult* __restrict__ total, uint32_t n,
    const uint8_t* __restrict__ slots, uint8_t* __restrict__ out) {
  if (total->res != lzenc::kOk) return;  // nothing is written: total <= out_cap holds below
  const uint32_t b = blockIdx.x, t = threadIdx.x;
  if (b == 0 && t == 0) out[offsets[n]] = 0;
  if (b >= n) return;
  const uint64_t len = results[b].dest_len;
  const uint8_t* s = slots + descs[b].dst_off;
  uint8_t* d = out + offsets[b];
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
  if (head > len) head = len;
  const uint64_t vecs = (len - head) >> 4;
  const uint64_t tail_at = head + (vecs << 4);
  for (uint64_t i = t; i < head; i += kMoveThreads) d[i] = s[i];
  for (uint64_t i = tail_at + t; i < len; i += kMoveThreads) d[i] = s[i];
  // d + head is 16-byte aligned; s + head is `sh` bytes into an aligned 16
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s + head);
  const uint32_t sh = uint32_t(sa & 15);
  const uint4* sv = reinterpret_cast<const uint4*>(sa - sh);
  uint4* dv = reinterpret_cast<uint4*>(d + head);
  if (sh == 0) {
    for (uint64_t i = t; i < vecs; i += kMoveThreads) dv[i] = sv[i];
    return;
  }
  // the second load's 16 bytes hold the vector's last source byte, so both
  // loads stay inside aligned 16-byte granules that the slot itself touches
  const uint32_t word = sh >> 2, bits = (sh & 3) * 8;
  for (uint64_t i = t; i < vecs; i += kMoveThreads) {
    const uint4 a = sv[i], c = sv[i + 1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    uint4 v;
    switch (word) {  // uniform over the block
      case 0:
        v = make_uint4(funnel(w[0], w[1], bits), funnel(w[1], w[2], bits),
                       funnel(w[2], w[3], bits), funnel(w[3], w[4], bits));
        break;
      case 1:
        v = make_uint4(funnel(w[1], w[2], bits), funnel(w[2], w[3], bits),
                       funnel(w[3], w[4], bits), funnel(w[4], w[5], bits));
        break;
      case 2:
        v = make_uint4(funnel(w[2], w[3], bits), funnel(w[3], w[4], bits),
                       funnel(w[4], w[5], bits), funnel(w[5], w[6], bits));
        break;
      default:
        v = make_uint4(funnel(w[3], w[4], bits), funnel(w[4], w[5], bits),
                       funnel(w[5], w[6], bits), funnel(w[6], w[7], bits));
        break;
    }
    dv[i] = v;
  }
}

}  // namespace

extern "C" int lzma2encgpu_launch(const LzmaEncGpuStreamDesc* d_descs, const uint32_t* d_order,
                                  uint32_t first, uint32_t count, uint32_t n,
                                  const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_ws,
                                  LzmaEncGpuResult* d_results, uint32_t lanes,
                                  hipStream_t stream, uint32_t kernels) {
  if (count == 0) return 0;
  if (lanes != 0 && lanes != 16 && lanes != 32 && lanes != 64) return -2;
  if (first > n || count > n - first) return -2;
  // at least ~4,096 workgroups of 256 for the clear, at most 64 parts a block
  uint32_t parts = (4096 + count - 1) / count;
  if (parts > 64) parts = 64;
  if (parts < 1) parts = 1;
  const uint64_t want = uint64_t(count) * parts;
  const uint32_t grid = uint32_t(want < 65536 ? want : 65536);
  hipLaunchKernelGGL(lzma2enc_init_kernel, dim3(grid), dim3(kInitThreads), 0, stream, d_descs,
                     d_order, first, count, n, parts, d_ws);
  if (hipGetLastError() != hipSuccess) return -1;
  if ((kernels & kLzmaEncKernelNormal) &&
      lzma2encgpu_launch_normal(d_descs, d_order, first, count, n, d_src, d_dst, d_ws, d_results,
                                lanes ? lanes : kLzmaEncLanesNormalDefault, stream) != 0)
    return -1;
  if (kernels & kLzmaEncKernelFast) {
    const uint32_t lf = lanes ? lanes : kLzmaEncLanesDefault;
    const uint32_t groups = uint32_t((uint64_t(count) + lf - 1) / lf);
    hipLaunchKernelGGL(lzma2enc_encode_kernel, dim3(groups), dim3(64), 0, stream, d_descs, d_order,
                       first, count, n, lf, d_src, d_dst, d_ws, d_results);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return 0;
}

extern "C" int lzma2encgpu_launch_compact(const LzmaEncGpuStreamDesc* d_descs,
                                          const LzmaEncGpuResult* d_results, uint32_t n,
                                          const uint8_t* d_slots, uint8_t* d_out, uint64_t out_cap,
                                          uint64_t* d_offsets, LzmaEncGpuResult* d_total,
                                          hipStream_t stream) {
  hipLaunchKernelGGL(lzma2enc_scan_kernel, dim3(1), dim3(kMoveThreads), 0, stream, d_results, n,
                     out_cap, d_offsets, d_total);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(lzma2enc_compact_kernel, dim3(n ? n : 1), dim3(kMoveThreads), 0, stream,
                     d_descs, d_results, d_offsets, d_total, n, d_slots, d_out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
