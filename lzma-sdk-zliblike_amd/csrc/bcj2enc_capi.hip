// bcj2enc_capi.hip -- C ABI of the BCJ2 batch encoder (include/lzma_gpu.h): the
// bounds, the scratch size, the device batch call and the host batch call
// through the host batch driver.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/lzma_gpu.h"
#include "bcj2enc_device.h"
#include "bcj2enc_internal.h"
#include "host_batch.h"
#include "lzma_gpu_internal.h"

using namespace lzgpu_host;

static_assert(sizeof(Bcj2GpuEncDesc) == 80 && sizeof(Bcj2GpuEncResult) == 40, "BCJ2 encode ABI");
static_assert(sizeof(bcj2enc::Info) == 64 && sizeof(bcj2enc::Header) == 64 &&
                  sizeof(bcj2enc::Elem) == 20 && sizeof(bcj2enc::SegBase) == 16,
              "BCJ2 encode scratch layout");

extern "C" void Bcj2EncGpu_Bound(uint64_t src_len, uint64_t bound[4]) {
  bound[LZMA_GPU_BCJ2_MAIN] = src_len;
  bound[LZMA_GPU_BCJ2_CALL] = bound[LZMA_GPU_BCJ2_JUMP] = 4 * (src_len / 5);
  bound[LZMA_GPU_BCJ2_RC] = 5 + src_len;
}

extern "C" uint64_t Bcj2EncGpu_Scratch(const Bcj2GpuEncDesc* descs, size_t n) {
  uint64_t bytes = bcj2enc::fixed_bytes();
  for (size_t i = 0; i < n; ++i) bytes += bcj2enc::slice_bytes(descs[i].src_len);
  return bytes;
}

extern "C" SRes Bcj2EncGpu_EncodeBatch(const Bcj2GpuEncDesc* d_descs, size_t n, const Byte* d_src,
                                       Byte* d_dst, void* d_scratch, Bcj2GpuEncResult* d_results,
                                       void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (bcj2encgpu_launch(d_descs, uint32_t(n), d_src, d_dst, static_cast<uint8_t*>(d_scratch),
                        d_results, kBcj2EncAll, static_cast<hipStream_t>(stream)) != 0) {
    set_error("BCJ2 encode batch kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

extern "C" SRes Bcj2EncGpu_EncodeBatchHost(const Bcj2GpuEncDesc* descs, size_t n, const Byte* src,
                                           size_t src_size, Byte* dst, size_t dst_size,
                                           Bcj2GpuEncResult* results, uint64_t workspace_limit) {
  static const char what[] = "BCJ2 encode batch";
  return guarded("BCJ2 encode batch: host allocation failed", [&]() -> SRes {
    if (!ensure_device()) return SZ_ERROR_FAIL;
    if (n == 0) return SZ_OK;
    HostBatch<Bcj2GpuEncDesc, Bcj2GpuEncResult> b;
    b.ws_fixed = bcj2enc::fixed_bytes();
    SRes r = b.lay_out_ranges(
        what, descs, n, workspace_limit,
        [&](const Bcj2GpuEncDesc& d) {
          if (d.src_off > src_size || d.src_len > src_size - d.src_off) return false;
          for (const Bcj2GpuEncRange& o : d.out)
            if (o.off > dst_size || o.cap > dst_size - o.off) return false;
          return true;
        },
        [](const Bcj2GpuEncDesc& d) { return d.src_len; },
        [](const Bcj2GpuEncDesc& d) { return bcj2enc::slice_bytes(d.src_len); });
    if (r != SZ_OK) return r;
    r = b.queue(what, in_plan_order(descs, b.plan), false, src, src_size, dst, dst_size,
                [&](uint32_t lo, uint32_t cnt) {
                  return bcj2encgpu_launch(b.desc.p + lo, cnt, b.src.p, b.dst.p, b.ws.p,
                                           b.res.p + lo, kBcj2EncAll, nullptr);
                });
    if (r != SZ_OK || (r = b.wait_scattered(what, results)) != SZ_OK) return r;
    return b.download_dst(dst, 0, dst_size) ? SZ_OK : SZ_ERROR_FAIL;
  });
}
