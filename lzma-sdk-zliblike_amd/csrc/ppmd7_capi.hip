// ppmd7_capi.hip -- C ABI of the PPMd7 batch decoder and encoder (include/lzma_gpu.h).
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/lzma_gpu.h"
#include "host_batch.h"
#include "lzma_gpu_internal.h"
#include "ppmd7_internal.h"

using namespace lzgpu_host;

static bool props_ok(uint32_t order, uint32_t mem_size) {
  return order >= 2 && order <= 64 && mem_size >= (1u << 11) && mem_size <= 0xFFFFFFFFu - 36u;
}

extern "C" uint64_t Ppmd7Gpu_WorkspaceBytes(uint32_t mem_size) {
  return props_ok(6, mem_size) ? ppmd7_slice_bytes(mem_size) : 0;
}

extern "C" SRes Ppmd7Gpu_DecodeBatch(const Ppmd7GpuStreamDesc* d_descs, size_t n,
                                     const Byte* d_src, Byte* d_dst, void* d_workspace,
                                     Ppmd7GpuResult* d_results, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (n == 0) return SZ_OK;
  if (ppmd7gpu_launch(d_descs, uint32_t(n), d_src, d_dst, static_cast<uint8_t*>(d_workspace),
                      d_results, static_cast<hipStream_t>(stream)) != 0) {
    set_error("PPMd7 batch kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

extern "C" SRes Ppmd7Gpu_EncodeBatch(const Ppmd7GpuEncDesc* d_descs, size_t n, const Byte* d_src,
                                     Byte* d_dst, void* d_workspace,
                                     Ppmd7GpuEncResult* d_results, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (n == 0) return SZ_OK;
  if (ppmd7encgpu_launch(d_descs, uint32_t(n), d_src, d_dst, static_cast<uint8_t*>(d_workspace),
                         d_results, static_cast<hipStream_t>(stream)) != 0) {
    set_error("PPMd7 batch kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

// The host call of either direction.  Desc is Ppmd7GpuStreamDesc or
// Ppmd7GpuEncDesc (one layout); dst_bytes(d) is the stream's range in dst,
// work(d) what its run time grows with, launch the direction's kernel launcher.
template <class Desc, class Res, class DstBytes, class Work, class Launch>
static SRes batch_host(const Desc* descs, size_t n, const Byte* src, size_t src_size, Byte* dst,
                       size_t dst_size, Res* results, uint64_t workspace_limit,
                       DstBytes dst_bytes, Work work, Launch launch) {
  static const char what[] = "PPMd7 batch";
  return guarded("PPMd7 batch: host allocation failed", [&]() -> SRes {
    if (!ensure_device()) return SZ_ERROR_FAIL;
    if (n == 0) return SZ_OK;
    HostBatch<Desc, Res> b;
    SRes r = b.lay_out(what, descs, n, src_size, dst_size, workspace_limit, dst_bytes, work,
                       [](const Desc& d) -> uint64_t {
                         return props_ok(d.order, d.mem_size) ? ppmd7_slice_bytes(d.mem_size) : 0;
                       });
    if (r != SZ_OK) return r;
    r = b.queue(what, in_launch_order(descs, b.plan), false, src, src_size, dst, dst_size,
                [&](uint32_t lo, uint32_t cnt) {
                  return launch(b.desc.p + lo, cnt, b.src.p, b.dst.p, b.ws.p, b.res.p + lo, nullptr);
                });
    if (r != SZ_OK || (r = b.wait_scattered(what, results)) != SZ_OK) return r;
    return b.download_dst(dst, 0, dst_size) ? SZ_OK : SZ_ERROR_FAIL;
  });
}

extern "C" SRes Ppmd7Gpu_DecodeBatchHost(const Ppmd7GpuStreamDesc* descs, size_t n, const Byte* src,
                                         size_t src_size, Byte* dst, size_t dst_size,
                                         Ppmd7GpuResult* results, uint64_t workspace_limit) {
  const auto len = [](const Ppmd7GpuStreamDesc& d) { return d.dst_len; };
  return batch_host(descs, n, src, src_size, dst, dst_size, results, workspace_limit, len, len,
                    ppmd7gpu_launch);
}

extern "C" SRes Ppmd7Gpu_EncodeBatchHost(const Ppmd7GpuEncDesc* descs, size_t n, const Byte* src,
                                         size_t src_size, Byte* dst, size_t dst_size,
                                         Ppmd7GpuEncResult* results, uint64_t workspace_limit) {
  return batch_host(
      descs, n, src, src_size, dst, dst_size, results, workspace_limit,
      [](const Ppmd7GpuEncDesc& d) { return d.dst_cap; },
      [](const Ppmd7GpuEncDesc& d) { return d.src_len; }, ppmd7encgpu_launch);
}
