// ppmd7_kernels.hip -- PPMd7 batch decode: one stream per 64-lane wave, one wave
// per workgroup.  Every lane runs ppmd7_device.h's decoder on the same state
// (wave-uniform control flow; the lanes store identical values to identical
// addresses, as in lzgpu_decode_dup_kernel), except for the bulk
// initialisations, which are dealt over the lanes.  The model and BinSumm live
// in the stream's workspace slice; the hot tables (Ppmd7Hot: charMask, the
// candidate list, SEE, the free lists, the small lookup tables, 3.5 KiB) live
// in LDS.  BinSumm (16 KiB) in LDS was measured and dropped: no faster at 64
// and 1,024 streams, and at 4,096 its 20 KiB per workgroup halves the resident
// waves (profiles/ppmd7/binsumm_ab.jsonl).
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "lzma_device.h"
#include "lzma_gpu_internal.h"
#include "ppmd7_device.h"
#include "ppmd7_internal.h"

__global__ void __launch_bounds__(64) ppmd7_decode_kernel(
    const Ppmd7GpuStreamDesc* __restrict__ descs, uint32_t n, const uint8_t* __restrict__ src,
    uint8_t* __restrict__ dst, uint8_t* __restrict__ ws, Ppmd7GpuResult* __restrict__ results) {
  __shared__ Ppmd7Hot hot;
  const uint32_t id = blockIdx.x;
  if (id >= n) return;
  {
    Ppmd7 t;
    t.h = &hot;
    t.build_tables();
  }
  const Ppmd7GpuStreamDesc d = descs[id];
  // keep the shared decoder state in vector registers (lz_vzero)
  const uint32_t z = lzgpu::lz_vzero();
  uint8_t* model = ws + d.ws_off + z;
  uint16_t* bin = (uint16_t*)(model + ppmd7_bin_offset(d.mem_size));
  const Ppmd7Out r = ppmd7_decode_stream(src + d.src_off + z, d.src_len, dst + d.dst_off + z,
                                         d.dst_len, d.order, d.mem_size, model, &hot, bin,
                                         threadIdx.x, 64);
  if (threadIdx.x == 0) {
    Ppmd7GpuResult o;
    o.res = r.res;
    o._pad = 0;
    o.dest_len = r.dest_len;
    o.src_len = r.src_len;
    results[id] = o;
  }
}

extern "C" int ppmd7gpu_launch(const Ppmd7GpuStreamDesc* d_descs, uint32_t n, const uint8_t* d_src,
                               uint8_t* d_dst, uint8_t* d_ws, Ppmd7GpuResult* d_results,
                               hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(ppmd7_decode_kernel, dim3(n), dim3(64), 0, stream, d_descs, n, d_src, d_dst,
                     d_ws, d_results);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
