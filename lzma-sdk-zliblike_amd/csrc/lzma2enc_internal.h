// lzma2enc_internal.h -- the LZMA2 encode launchers, shared by
// lzma2enc_kernels.hip and lzma2enc_capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lzma_gpu.h"
#include "lzma2enc_device.h"
#include "lzmaenc_internal.h"

// what the kernel ends a block with before touching memory
__host__ __device__ inline int32_t lzma2enc_check(const LzmaEncGpuStreamDesc& d) {
  if (d.mode > (LZMA_ENC_GPU_MODE_OPTIMAL | LZMA_ENC_GPU_MODE_BT4)) return lzenc::kErrParam;
  const int32_t r = lzenc::lzma2_check_params(lzmaenc_params(d), d.src_len);
  if (r != lzenc::kOk) return r;
  return (d.ws_off & 15u) ? lzenc::kErrParam : lzenc::kOk;
}
// a block's workspace slice in bytes, wherever it is put; 0 for a descriptor
// the kernel refuses with its own per-block code
inline uint64_t lzma2enc_slice_bytes(const LzmaEncGpuStreamDesc& d) {
  LzmaEncGpuStreamDesc t = d;
  t.ws_off = 0;
  if (lzma2enc_check(t) != lzenc::kOk) return 0;
  return lzenc::lzma2enc_layout(lzmaenc_params(t), t.src_len).bytes;
}

// Launches on `stream` over blocks order[first, first + count) of the n
// descriptors (order null: index order): the grid clears every block's hash
// and sets its probability cells, then one lane per block encodes (lanes
// blocks per wave: 16, 32, 64, or 0 for each kernel's default) in the kernels
// of `kernels` (lzmaenc_internal.h's kLzmaEncKernel* bits).  Results land at
// the block's own index.  0 on success.
extern "C" int lzma2encgpu_launch(const LzmaEncGpuStreamDesc* d_descs, const uint32_t* d_order,
                                  uint32_t first, uint32_t count, uint32_t n,
                                  const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_ws,
                                  LzmaEncGpuResult* d_results, uint32_t lanes,
                                  hipStream_t stream,
                                  uint32_t kernels = kLzmaEncKernelFast | kLzmaEncKernelNormal);
// The normal-mode block encode kernel alone (lzma2enc_normal_kernels.hip).
extern "C" int lzma2encgpu_launch_normal(const LzmaEncGpuStreamDesc* d_descs,
                                         const uint32_t* d_order, uint32_t first, uint32_t count,
                                         uint32_t n, const uint8_t* d_src, uint8_t* d_dst,
                                         uint8_t* d_ws, LzmaEncGpuResult* d_results,
                                         uint32_t lanes, hipStream_t stream);
// Two launches: the scan of the blocks' dest_len into d_offsets (n + 1) and
// d_total, then the gather of every block from d_slots + descs[i].dst_off to
// d_out + d_offsets[i] and the final 0x00.  Nothing is written to d_out unless
// d_total->res is SZ_OK.  0 on success.
extern "C" int lzma2encgpu_launch_compact(const LzmaEncGpuStreamDesc* d_descs,
                                          const LzmaEncGpuResult* d_results, uint32_t n,
                                          const uint8_t* d_slots, uint8_t* d_out, uint64_t out_cap,
                                          uint64_t* d_offsets, LzmaEncGpuResult* d_total,
                                          hipStream_t stream);
