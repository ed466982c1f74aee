// lzmaenc_capi.hip -- C ABI of the LZMA fast-mode batch encoder
// (include/lzma_gpu.h): the props drop-ins, descriptor and workspace planning,
// the device and host batch calls, and LzmaEncode / LzmaCompress as one-item
// calls of the host form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <exception>
#include <numeric>
#include <string.h>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "lzma_gpu_internal.h"
#include "lzmaenc_device.h"
#include "lzmaenc_internal.h"

using namespace lzgpu_host;

static_assert(sizeof(CLzmaEncProps) == 48 && sizeof(lzenc::EncProps) == sizeof(CLzmaEncProps),
              "CLzmaEncProps layout (LzmaEnc.h:15-31)");
static_assert(sizeof(LzmaEncGpuStreamDesc) == 72 && sizeof(LzmaEncGpuResult) == 16, "encode ABI");

static lzenc::EncProps to_enc(const CLzmaEncProps* p) {
  lzenc::EncProps e;
  memcpy(&e, p, sizeof(e));
  return e;
}

extern "C" void LzmaEncProps_Init(CLzmaEncProps* p) {
  lzenc::EncProps e;
  lzenc::props_init(&e);
  memcpy(p, &e, sizeof(e));
}

extern "C" void LzmaEncProps_Normalize(CLzmaEncProps* p) {
  lzenc::EncProps e = to_enc(p);
  lzenc::props_normalize(&e);
  memcpy(p, &e, sizeof(e));
}

extern "C" UInt32 LzmaEncProps_GetDictSize(const CLzmaEncProps* props2) {
  lzenc::EncProps e = to_enc(props2);
  lzenc::props_normalize(&e);
  return e.dictSize;
}

static const char kNotFastPath[] =
    "LZMA encode: props normalise to the optimal parser (algo 1) or a bt match finder "
    "(btMode 1); only the fast path (levels 0..4: algo 0, btMode 0) is built";

extern "C" SRes LzmaEncGpu_DescFromProps(const CLzmaEncProps* props, int writeEndMark,
                                         LzmaEncGpuStreamDesc* desc, Byte props5[5]) {
  const lzenc::EncProps e = to_enc(props);
  lzenc::Params q;
  const int32_t r = lzenc::params_from_props(&e, writeEndMark, &q);
  if (r == lzenc::kErrUnsupported) set_error(kNotFastPath);
  if (r != lzenc::kOk) return r;
  desc->dict_size = q.dict_size;
  desc->lc = q.lc;
  desc->lp = q.lp;
  desc->pb = q.pb;
  desc->fb = q.fb;
  desc->mc = q.mc;
  desc->write_end_mark = q.write_end_mark;
  desc->reserved = 0;
  lzenc::write_props5(q, props5);
  return SZ_OK;
}

static uint64_t slice_bytes(const LzmaEncGpuStreamDesc& d) {
  LzmaEncGpuStreamDesc t = d;
  t.ws_off = 0;
  if (lzmaenc_check(t) != lzenc::kOk) return 0;
  return lzenc::lzmaenc_layout(lzmaenc_params(t), t.src_len).bytes;
}

static void longest_first(const LzmaEncGpuStreamDesc* descs, size_t n, uint32_t* order) {
  std::iota(order, order + n, 0u);
  std::stable_sort(order, order + n,
                   [&](uint32_t a, uint32_t b) { return descs[a].src_len > descs[b].src_len; });
}

static SRes plan_batch(LzmaEncGpuStreamDesc* descs, size_t n, uint32_t* order,
                       uint64_t* workspace_bytes) {
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  uint64_t at = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t need = slice_bytes(descs[i]);
    descs[i].ws_off = need ? at : 0;
    at += need;
  }
  if (workspace_bytes) *workspace_bytes = at;
  if (order) longest_first(descs, n, order);
  return SZ_OK;
}

extern "C" SRes LzmaEncGpu_PlanBatch(LzmaEncGpuStreamDesc* descs, size_t n, uint32_t* order,
                                     uint64_t* workspace_bytes) {
  try {
    return plan_batch(descs, n, order, workspace_bytes);
  } catch (const std::exception&) {
    set_error("LZMA encode plan: host allocation failed");
    return SZ_ERROR_MEM;
  }
}

extern "C" SRes LzmaEncGpu_EncodeBatch(const LzmaEncGpuStreamDesc* d_descs, const uint32_t* d_order,
                                       size_t n, const Byte* d_src, Byte* d_dst, void* d_workspace,
                                       LzmaEncGpuResult* d_results, unsigned lanes, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (lanes == LZMA_ENC_GPU_LANES_DEFAULT) lanes = kLzmaEncLanesDefault;
  if (lanes != 16 && lanes != 32 && lanes != 64) return SZ_ERROR_PARAM;
  if (n == 0) return SZ_OK;
  if (lzmaencgpu_launch(d_descs, d_order, uint32_t(n), d_src, d_dst,
                        static_cast<uint8_t*>(d_workspace), d_results, lanes,
                        static_cast<hipStream_t>(stream)) != 0) {
    set_error("LZMA encode batch kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

// one_item: dst is not uploaded and only [0, dest_len) comes back (the drop-ins'
// dest may be far larger than the stream)
static SRes encode_batch_host(const LzmaEncGpuStreamDesc* descs, size_t n, const Byte* src,
                              size_t src_size, Byte* dst, size_t dst_size,
                              LzmaEncGpuResult* results, uint64_t workspace_limit, bool one_item) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n == 0) return SZ_OK;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  for (size_t i = 0; i < n; ++i) {
    const LzmaEncGpuStreamDesc& d = descs[i];
    if (d.src_off > src_size || d.src_len > src_size - d.src_off || d.dst_off > dst_size ||
        d.dst_cap > dst_size - d.dst_off)
      return SZ_ERROR_PARAM;
  }
  if (workspace_limit == 0) {
    size_t free_b = 0, total_b = 0;
    if (!hip_ok(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo")) return SZ_ERROR_FAIL;
    workspace_limit = free_b / 2;
  }
  // longest first: the waves of a launch start in index order
  std::vector<uint32_t> order(n);
  longest_first(descs, n, order.data());
  // launches: consecutive streams of the order while their slices fit the limit
  std::vector<LzmaEncGpuStreamDesc> d(n);
  std::vector<size_t> cut{0};
  uint64_t ws_max = 0, ws_cur = 0;
  for (size_t k = 0; k < n; ++k) {
    d[k] = descs[order[k]];
    const uint64_t need = slice_bytes(d[k]);
    if (need > workspace_limit) {
      set_error("LZMA encode batch: one stream's workspace slice exceeds the limit");
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
  DevArr<LzmaEncGpuStreamDesc> g_desc;
  DevArr<LzmaEncGpuResult> g_res;
  if (!g_src.alloc(src_size) || !g_dst.alloc(dst_size) || !g_ws.alloc(ws_max) ||
      !g_desc.alloc(n) || !g_res.alloc(n)) {
    (void)hipGetLastError();
    set_error("LZMA encode batch: device allocation failed");
    return SZ_ERROR_MEM;
  }
  if (!hip_ok(hipMemcpy(g_src.p, src, src_size, hipMemcpyHostToDevice), "upload src") ||
      (!one_item &&
       !hip_ok(hipMemcpy(g_dst.p, dst, dst_size, hipMemcpyHostToDevice), "upload dst")) ||
      !hip_ok(hipMemcpy(g_desc.p, d.data(), n * sizeof(d[0]), hipMemcpyHostToDevice),
              "upload descs"))
    return SZ_ERROR_FAIL;
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    const size_t lo = cut[c], cnt = cut[c + 1] - lo;
    if (cnt == 0) continue;
    if (lzmaencgpu_launch(g_desc.p + lo, nullptr, uint32_t(cnt), g_src.p, g_dst.p, g_ws.p,
                          g_res.p + lo, kLzmaEncLanesDefault, nullptr) != 0) {
      set_error("LZMA encode batch kernel launch failed");
      return SZ_ERROR_FAIL;
    }
  }
  std::vector<LzmaEncGpuResult> r(n);
  if (!hip_ok(hipDeviceSynchronize(), "LZMA encode batch") ||
      !hip_ok(hipMemcpy(r.data(), g_res.p, n * sizeof(r[0]), hipMemcpyDeviceToHost),
              "download results"))
    return SZ_ERROR_FAIL;
  if (one_item) {
    const uint64_t len = std::min<uint64_t>(r[0].dest_len, d[0].dst_cap);
    if (len && !hip_ok(hipMemcpy(dst + d[0].dst_off, g_dst.p + d[0].dst_off, len,
                                 hipMemcpyDeviceToHost), "download dst"))
      return SZ_ERROR_FAIL;
  } else if (!hip_ok(hipMemcpy(dst, g_dst.p, dst_size, hipMemcpyDeviceToHost), "download dst")) {
    return SZ_ERROR_FAIL;
  }
  for (size_t k = 0; k < n; ++k) results[order[k]] = r[k];
  return SZ_OK;
}

extern "C" SRes LzmaEncGpu_EncodeBatchHost(const LzmaEncGpuStreamDesc* descs, size_t n,
                                           const Byte* src, size_t src_size, Byte* dst,
                                           size_t dst_size, LzmaEncGpuResult* results,
                                           uint64_t workspace_limit) {
  try {
    return encode_batch_host(descs, n, src, src_size, dst, dst_size, results, workspace_limit,
                             false);
  } catch (const std::exception&) {
    set_error("LZMA encode batch: host allocation failed");
    return SZ_ERROR_MEM;
  }
}

extern "C" SRes LzmaEncode(Byte* dest, SizeT* destLen, const Byte* src, SizeT srcLen,
                           const CLzmaEncProps* props, Byte* propsEncoded, SizeT* propsSize,
                           int writeEndMark, ICompressProgress* progress, ISzAlloc* alloc,
                           ISzAlloc* allocBig) {
  (void)progress;
  (void)alloc;
  (void)allocBig;
  // LzmaEnc_SetProps, then LzmaEnc_WriteProperties' size check, then what this
  // library does not encode
  const lzenc::EncProps e = to_enc(props);
  lzenc::Params q;
  const int32_t pr = lzenc::params_from_props(&e, writeEndMark, &q);
  if (pr == lzenc::kErrParam) return SZ_ERROR_PARAM;
  if (*propsSize < LZMA_PROPS_SIZE) return SZ_ERROR_PARAM;
  if (pr == lzenc::kErrUnsupported) {
    set_error(kNotFastPath);
    return SZ_ERROR_UNSUPPORTED;
  }
  if (uint64_t(srcLen) >= (uint64_t(1) << 31)) {
    set_error("LZMA encode: a source of 2^31 bytes or more is not supported");
    return SZ_ERROR_UNSUPPORTED;
  }
  if (!ensure_device()) return SZ_ERROR_FAIL;
  *propsSize = LZMA_PROPS_SIZE;
  lzenc::write_props5(q, propsEncoded);
  LzmaEncGpuStreamDesc d;
  memset(&d, 0, sizeof(d));
  d.src_len = srcLen;
  d.dst_cap = *destLen;
  d.dict_size = q.dict_size;
  d.lc = q.lc;
  d.lp = q.lp;
  d.pb = q.pb;
  d.fb = q.fb;
  d.mc = q.mc;
  d.write_end_mark = q.write_end_mark;
  LzmaEncGpuResult r;
  r.res = SZ_ERROR_FAIL;
  r.dest_len = 0;
  SRes res;
  try {
    res = encode_batch_host(&d, 1, src, srcLen, dest, *destLen, &r, 0, true);
  } catch (const std::exception&) {
    set_error("LZMA encode: host allocation failed");
    return SZ_ERROR_MEM;
  }
  if (res != SZ_OK) return res;
  *destLen = SizeT(r.dest_len);
  return r.res;
}

extern "C" int LzmaCompress(unsigned char* dest, size_t* destLen, const unsigned char* src,
                            size_t srcLen, unsigned char* outProps, size_t* outPropsSize,
                            int level, unsigned dictSize, int lc, int lp, int pb, int fb,
                            int numThreads) {
  CLzmaEncProps props;
  LzmaEncProps_Init(&props);
  props.level = level;
  props.dictSize = dictSize;
  props.lc = lc;
  props.lp = lp;
  props.pb = pb;
  props.fb = fb;
  props.numThreads = numThreads;
  return LzmaEncode(dest, destLen, src, srcLen, &props, outProps, outPropsSize, 0, nullptr, nullptr,
                    nullptr);
}
