// ppmd7enc_kernels.hip -- PPMd7 batch encode, the decode kernel's shape: one
// stream per 64-lane wave, one wave per workgroup.  Every lane runs
// ppmd7_device.h's encoder on the same state (wave-uniform control flow; the
// lanes store identical values to identical addresses), except for the bulk
// initialisations, which are dealt over the lanes, and the searches of a
// context's states for the symbol, one state per lane (scan_states).  The model
// and BinSumm live in the stream's workspace slice, laid out as for decoding;
// the hot tables (Ppmd7Hot) live in LDS.
//
// amdgpu_waves_per_eu(4, 4): left alone the compiler takes 142 VGPRs, three
// waves per SIMD, and 4,096 streams no longer fit the device at once; held to
// four it needs 127, still without scratch (PPMd7 encoding).
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "lzma_device.h"
#include "lzma_gpu_internal.h"
#include "ppmd7_device.h"
#include "ppmd7_internal.h"

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
ppmd7_encode_kernel(
    const Ppmd7GpuEncDesc* __restrict__ descs, uint32_t n, const uint8_t* __restrict__ src,
    uint8_t* __restrict__ dst, uint8_t* __restrict__ ws, Ppmd7GpuEncResult* __restrict__ results) {
  __shared__ Ppmd7Hot hot;
  const uint32_t id = blockIdx.x;
  if (id >= n) return;
  {
    Ppmd7 t;
    t.h = &hot;
    t.build_tables();
  }
  const Ppmd7GpuEncDesc d = descs[id];
  // keep the shared encoder state in vector registers (lz_vzero)
  const uint32_t z = lzgpu::lz_vzero();
  uint8_t* model = ws + d.ws_off + z;
  uint16_t* bin = (uint16_t*)(model + ppmd7_bin_offset(d.mem_size));
  const Ppmd7EncOut r = ppmd7_encode_stream(src + d.src_off + z, d.src_len, dst + d.dst_off + z,
                                            d.dst_cap, d.order, d.mem_size, model, &hot, bin,
                                            threadIdx.x, 64);
  if (threadIdx.x == 0) {
    Ppmd7GpuEncResult o;
    o.res = r.res;
    o._pad = 0;
    o.dest_len = r.dest_len;
    o.packed_len = r.packed_len;
    results[id] = o;
  }
}

extern "C" int ppmd7encgpu_launch(const Ppmd7GpuEncDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                  uint8_t* d_dst, uint8_t* d_ws, Ppmd7GpuEncResult* d_results,
                                  hipStream_t stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(ppmd7_encode_kernel, dim3(n), dim3(64), 0, stream, d_descs, n, d_src, d_dst,
                     d_ws, d_results);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
