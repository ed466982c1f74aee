// lzmaenc_internal.h -- the LZMA encode launcher, shared by lzmaenc_kernels.hip
// and lzmaenc_capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lzma_gpu.h"
#include "lzmaenc_device.h"

// Streams per 64-lane wave when the caller leaves the choice to the library.
// One stream per lane diverges at every token, so a wave's time is the sum of
// its lanes' distinct paths: fewer lanes per wave trade idle lanes for shorter
// waves.  Measured (profiles/lzmaenc/lanes_ab.jsonl, level 1, two alternating
// rounds): 16 lanes beat 32 and 64 at every batch size -- 65,536 x 4 KiB
// 1,651 / 1,462 / 1,355 MB/s, 4,096 x 4 KiB 320 / 239 / 185, 4,096 x 64 KiB
// 325 / 252 / 198, 64 x 4 KiB 6.5 / 4.8 / 3.6; one stream is 0.52 MB/s at any.
constexpr uint32_t kLzmaEncLanesDefault = 16;

__host__ __device__ inline lzenc::Params lzmaenc_params(const LzmaEncGpuStreamDesc& d) {
  lzenc::Params q;
  q.dict_size = d.dict_size;
  q.lc = d.lc;
  q.lp = d.lp;
  q.pb = d.pb;
  q.fb = d.fb;
  q.mc = d.mc;
  q.write_end_mark = d.write_end_mark;
  return q;
}
// what the kernel ends a stream with before touching memory
__host__ __device__ inline int32_t lzmaenc_check(const LzmaEncGpuStreamDesc& d) {
  const int32_t r = lzenc::check_params(lzmaenc_params(d), d.src_len);
  if (r != lzenc::kOk) return r;
  return (d.ws_off & 15u) ? lzenc::kErrParam : lzenc::kOk;
}
// a stream's workspace slice in bytes, wherever it is put; 0 for a descriptor
// the kernel refuses with its own per-stream code
inline uint64_t lzmaenc_slice_bytes(const LzmaEncGpuStreamDesc& d) {
  LzmaEncGpuStreamDesc t = d;
  t.ws_off = 0;
  if (lzmaenc_check(t) != lzenc::kOk) return 0;
  return lzenc::lzmaenc_layout(lzmaenc_params(t), t.src_len).bytes;
}

// The first of the two launches alone (lzmaenc_bench.py times it separately).
extern "C" int lzmaencgpu_launch_init(const LzmaEncGpuStreamDesc* d_descs, uint32_t n,
                                      uint8_t* d_ws, hipStream_t stream);
// Two launches on `stream`: the grid clears every stream's hash and sets its
// probability cells, then one lane per stream encodes (lanes streams per wave:
// 16, 32 or 64).  0 on success.
extern "C" int lzmaencgpu_launch(const LzmaEncGpuStreamDesc* d_descs, const uint32_t* d_order,
                                 uint32_t n, const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_ws,
                                 LzmaEncGpuResult* d_results, uint32_t lanes, hipStream_t stream);
