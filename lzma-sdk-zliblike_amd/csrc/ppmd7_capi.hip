// ppmd7_capi.hip -- C ABI of the PPMd7 batch decoder and encoder (include/lzma_gpu.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <numeric>
#include <vector>

#include "../../include/lzma_gpu.h"
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
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n == 0) return SZ_OK;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  for (size_t i = 0; i < n; ++i) {
    const Desc& d = descs[i];
    if (d.src_off > src_size || d.src_len > src_size - d.src_off || d.dst_off > dst_size ||
        dst_bytes(d) > dst_size - d.dst_off)
      return SZ_ERROR_PARAM;
  }
  if (workspace_limit == 0) {
    size_t free_b = 0, total_b = 0;
    if (!hip_ok(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo")) return SZ_ERROR_FAIL;
    workspace_limit = free_b / 2;
  }
  // longest first: the workgroups of a launch start in index order
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return work(descs[a]) > work(descs[b]); });
  // launches: consecutive streams of the order while their slices fit the limit
  std::vector<Desc> d(n);
  std::vector<size_t> cut{0};
  uint64_t ws_max = 0, ws_cur = 0;
  for (size_t k = 0; k < n; ++k) {
    d[k] = descs[order[k]];
    const uint64_t need = props_ok(d[k].order, d[k].mem_size) ? ppmd7_slice_bytes(d[k].mem_size) : 0;
    if (need > workspace_limit) {
      set_error("PPMd7 batch: one stream's workspace slice exceeds the limit");
      return SZ_ERROR_MEM;
    }
    if (ws_cur + need > workspace_limit) {
      cut.push_back(k);
      ws_cur = 0;
    }
    d[k].ws_off = ws_cur;
    ws_cur += need;
    ws_max = std::max(ws_max, ws_cur);
  }
  cut.push_back(n);

  DevArr<uint8_t> g_src, g_dst, g_ws;
  DevArr<Desc> g_desc;
  DevArr<Res> g_res;
  if (!g_src.alloc(src_size) || !g_dst.alloc(dst_size) || !g_ws.alloc(ws_max) ||
      !g_desc.alloc(n) || !g_res.alloc(n)) {
    (void)hipGetLastError();
    set_error("PPMd7 batch: device allocation failed");
    return SZ_ERROR_MEM;
  }
  if (!hip_ok(hipMemcpy(g_src.p, src, src_size, hipMemcpyHostToDevice), "upload src") ||
      !hip_ok(hipMemcpy(g_dst.p, dst, dst_size, hipMemcpyHostToDevice), "upload dst") ||
      !hip_ok(hipMemcpy(g_desc.p, d.data(), n * sizeof(d[0]), hipMemcpyHostToDevice),
              "upload descs"))
    return SZ_ERROR_FAIL;
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    const size_t lo = cut[c], cnt = cut[c + 1] - lo;
    if (cnt == 0) continue;
    if (launch(g_desc.p + lo, uint32_t(cnt), g_src.p, g_dst.p, g_ws.p, g_res.p + lo, nullptr) != 0) {
      set_error("PPMd7 batch kernel launch failed");
      return SZ_ERROR_FAIL;
    }
  }
  std::vector<Res> r(n);
  if (!hip_ok(hipDeviceSynchronize(), "PPMd7 batch") ||
      !hip_ok(hipMemcpy(r.data(), g_res.p, n * sizeof(r[0]), hipMemcpyDeviceToHost),
              "download results") ||
      !hip_ok(hipMemcpy(dst, g_dst.p, dst_size, hipMemcpyDeviceToHost), "download dst"))
    return SZ_ERROR_FAIL;
  for (size_t k = 0; k < n; ++k) results[order[k]] = r[k];
  return SZ_OK;
}

extern "C" SRes Ppmd7Gpu_DecodeBatchHost(const Ppmd7GpuStreamDesc* descs, size_t n, const Byte* src,
                                         size_t src_size, Byte* dst, size_t dst_size,
                                         Ppmd7GpuResult* results, uint64_t workspace_limit) {
  try {
    const auto len = [](const Ppmd7GpuStreamDesc& d) { return d.dst_len; };
    return batch_host(descs, n, src, src_size, dst, dst_size, results, workspace_limit, len, len,
                      ppmd7gpu_launch);
  } catch (const std::exception&) {
    set_error("PPMd7 batch: host allocation failed");
    return SZ_ERROR_MEM;
  }
}

extern "C" SRes Ppmd7Gpu_EncodeBatchHost(const Ppmd7GpuEncDesc* descs, size_t n, const Byte* src,
                                         size_t src_size, Byte* dst, size_t dst_size,
                                         Ppmd7GpuEncResult* results, uint64_t workspace_limit) {
  try {
    return batch_host(
        descs, n, src, src_size, dst, dst_size, results, workspace_limit,
        [](const Ppmd7GpuEncDesc& d) { return d.dst_cap; },
        [](const Ppmd7GpuEncDesc& d) { return d.src_len; }, ppmd7encgpu_launch);
  } catch (const std::exception&) {
    set_error("PPMd7 batch: host allocation failed");
    return SZ_ERROR_MEM;
  }
}
