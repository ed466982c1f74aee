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
// The same choice for the normal-mode kernel, from the same alternating A/B
// (profiles/lzmaenc_opt/lanes_ab.jsonl, level 5, dictionary = stream size, two
// rounds): 16 lanes beat 32 and 64 -- 65,536 x 4 KiB 184.6 / 146.0 / 122.1 and
// 184.9 / 145.8 / 122.4 MB/s, 4,096 x 4 KiB 34.0 / 20.5 / 12.8 and 34.1 / 20.6 /
// 12.7.  Fewer than 16 was not measured.
constexpr uint32_t kLzmaEncLanesNormalDefault = 16;

__host__ __device__ inline lzenc::Params lzmaenc_params(const LzmaEncGpuStreamDesc& d) {
  lzenc::Params q;
  q.dict_size = d.dict_size;
  q.lc = d.lc;
  q.lp = d.lp;
  q.pb = d.pb;
  q.fb = d.fb;
  q.mc = d.mc;
  q.write_end_mark = d.write_end_mark;
  q.algo = (d.mode & LZMA_ENC_GPU_MODE_OPTIMAL) ? 1u : 0u;
  q.bt = (d.mode & LZMA_ENC_GPU_MODE_BT4) ? 1u : 0u;
  return q;
}
// what the kernel ends a stream with before touching memory
__host__ __device__ inline int32_t lzmaenc_check(const LzmaEncGpuStreamDesc& d) {
  if (d.mode > (LZMA_ENC_GPU_MODE_OPTIMAL | LZMA_ENC_GPU_MODE_BT4)) return lzenc::kErrParam;
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

// What a stream's place in the launch order grows with: the normal modes
// first, since they take longest (optimal parser with Bt4, with Hc4, then Bt4
// with the fast parser), and within a mode the longest source first.  With
// every stream at mode 0 this is src_len.
inline uint64_t lzmaenc_work(const LzmaEncGpuStreamDesc& d) {
  static const uint64_t rank[4] = {0, 2, 1, 3};
  const uint64_t len = d.src_len < (uint64_t(1) << 60) ? d.src_len : (uint64_t(1) << 60) - 1;
  return (d.mode <= 3 ? rank[d.mode] << 60 : 0) | len;
}
// Which encode kernels a batch of host-known descriptors needs: bit 0 the
// fast-path kernel (it also reports every stream the kernels reject), bit 1 the
// normal-mode kernel.
constexpr uint32_t kLzmaEncKernelFast = 1, kLzmaEncKernelNormal = 2;
template <class Check>
inline uint32_t lzmaenc_kernels(const LzmaEncGpuStreamDesc* descs, size_t n, Check check) {
  uint32_t k = 0;
  for (size_t i = 0; i < n && k != 3; ++i)
    k |= (descs[i].mode == 0 || check(descs[i]) != lzenc::kOk) ? kLzmaEncKernelFast
                                                                : kLzmaEncKernelNormal;
  return k;
}
// The process-wide mask of modes the props entry points may select
// (LzmaEncGpu_SetModes; lzmaenc_capi.hip).
uint32_t lzmaenc_allowed_modes();
// "<what>: props field <field> ..." as the last error of a refused props call
void lzmaenc_set_unsupported_error(const char* field);

// Encoder sessions (lzmaenc_session_kernels.hip, lzmaenc_session_capi.hip).
// A round's scratch, in 32-bit words: the header (the two counters, padded to
// 16 bytes), the work list (n indices), the init list (n indices).
constexpr uint32_t kLzmaEncSessionWorkCount = 0, kLzmaEncSessionInitCount = 1;
constexpr uint32_t kLzmaEncSessionHeaderWords = 4;
// The list pass alone (lzmaenc_session_bench.py times it separately): clears
// the counters, then compacts.
extern "C" int lzmaencgpu_session_launch_list(const LzmaEncGpuSession* d_sessions, uint32_t n,
                                              uint32_t* d_scratch, hipStream_t stream);
// One round on `stream`: list pass, init over the init list, encode over the
// work list (lanes 16, 32, 64, or 0 for kLzmaEncLanesDefault).  0 on success.
extern "C" int lzmaencgpu_session_launch(LzmaEncGpuSession* d_sessions, uint32_t n,
                                         uint32_t* d_scratch, uint32_t lanes, hipStream_t stream);

// The normal-mode encode kernel alone (lzmaenc_normal_kernels.hip); lanes 16, 32 or 64.
extern "C" int lzmaencgpu_launch_normal(const LzmaEncGpuStreamDesc* d_descs,
                                        const uint32_t* d_order, uint32_t n, const uint8_t* d_src,
                                        uint8_t* d_dst, uint8_t* d_ws, LzmaEncGpuResult* d_results,
                                        uint32_t lanes, hipStream_t stream);
// The first of the two launches alone (lzmaenc_bench.py times it separately).
extern "C" int lzmaencgpu_launch_init(const LzmaEncGpuStreamDesc* d_descs, uint32_t n,
                                      uint8_t* d_ws, hipStream_t stream);
// Launches on `stream`: the grid clears every stream's hash and sets its
// probability cells, then one lane per stream encodes (lanes streams per wave:
// 16, 32, 64, or 0 for each kernel's default) in the kernels of `kernels`
// (kLzmaEncKernel* bits; both when the descriptors are known to the device
// only).  Each kernel walks the same order and leaves the other's streams
// alone.  0 on success.
extern "C" int lzmaencgpu_launch(const LzmaEncGpuStreamDesc* d_descs, const uint32_t* d_order,
                                 uint32_t n, const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_ws,
                                 LzmaEncGpuResult* d_results, uint32_t lanes, hipStream_t stream,
                                 uint32_t kernels = kLzmaEncKernelFast | kLzmaEncKernelNormal);
