// lzmaenc_capi.hip -- C ABI of the LZMA batch encoder
// (include/lzma_gpu.h): the props drop-ins, descriptor and workspace planning,
// the device and host batch calls, and LzmaEncode / LzmaCompress as one-item
// calls of the host form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "host_batch.h"
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

// the process-wide mask: LZGPU_ENC_MODES (decimal) read once, then SetModes
static std::atomic<uint32_t>& allowed_modes() {
  static std::atomic<uint32_t> mask([] {
    const char* v = getenv("LZGPU_ENC_MODES");
    return v ? uint32_t(strtoul(v, nullptr, 10)) & 3u : 0u;
  }());
  return mask;
}
uint32_t lzmaenc_allowed_modes() { return allowed_modes().load(); }
extern "C" unsigned LzmaEncGpu_SetModes(unsigned allowed) {
  return allowed_modes().exchange(allowed & 3u);
}
extern "C" unsigned LzmaEncGpu_GetModes(void) { return lzmaenc_allowed_modes(); }

void lzmaenc_set_unsupported_error(const char* field) {
  const std::string f(field ? field : "algo");
  if (f == "numHashBytes")
    set_error("LZMA encode: props field numHashBytes selects the Bt2 or Bt3 match finder; of the "
              "bt finders only Bt4 (numHashBytes 4) is built");
  else
    set_error(("LZMA encode: props field " + f + " normalises to the optimal parser (algo 1) or "
               "the Bt4 match finder (btMode 1), which the mode mask does not allow "
               "(LzmaEncGpu_SetModes, LZGPU_ENC_MODES); mask 0 is the fast path alone "
               "(levels 0..4: algo 0, btMode 0)").c_str());
}

static void fill_desc(LzmaEncGpuStreamDesc* desc, const lzenc::Params& q) {
  desc->dict_size = q.dict_size;
  desc->lc = q.lc;
  desc->lp = q.lp;
  desc->pb = q.pb;
  desc->fb = q.fb;
  desc->mc = q.mc;
  desc->write_end_mark = q.write_end_mark;
  desc->mode = lzenc::mode_of(q);
}

extern "C" SRes LzmaEncGpu_DescFromPropsEx(const CLzmaEncProps* props, int writeEndMark,
                                           unsigned allowed, LzmaEncGpuStreamDesc* desc,
                                           Byte props5[5]) {
  const lzenc::EncProps e = to_enc(props);
  lzenc::Params q;
  const char* field = nullptr;
  const int32_t r = lzenc::params_from_props_ex(&e, writeEndMark, allowed, &q, &field);
  if (r == lzenc::kErrUnsupported) lzmaenc_set_unsupported_error(field);
  if (r != lzenc::kOk) return r;
  fill_desc(desc, q);
  lzenc::write_props5(q, props5);
  return SZ_OK;
}

extern "C" SRes LzmaEncGpu_DescFromProps(const CLzmaEncProps* props, int writeEndMark,
                                         LzmaEncGpuStreamDesc* desc, Byte props5[5]) {
  return LzmaEncGpu_DescFromPropsEx(props, writeEndMark, lzmaenc_allowed_modes(), desc, props5);
}

extern "C" SRes LzmaEncGpu_PlanBatch(LzmaEncGpuStreamDesc* descs, size_t n, uint32_t* order,
                                     uint64_t* workspace_bytes) {
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  return guarded("LZMA encode plan: host allocation failed", [&]() -> SRes {
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t need = lzmaenc_slice_bytes(descs[i]);
      descs[i].ws_off = need ? at : 0;
      at += need;
    }
    if (workspace_bytes) *workspace_bytes = at;
    if (order) longest_first(n, [&](uint32_t i) { return lzmaenc_work(descs[i]); }, order);
    return SZ_OK;
  });
}

extern "C" SRes LzmaEncGpu_EncodeBatch(const LzmaEncGpuStreamDesc* d_descs, const uint32_t* d_order,
                                       size_t n, const Byte* d_src, Byte* d_dst, void* d_workspace,
                                       LzmaEncGpuResult* d_results, unsigned lanes, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (lanes != LZMA_ENC_GPU_LANES_DEFAULT && lanes != 16 && lanes != 32 && lanes != 64)
    return SZ_ERROR_PARAM;
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
  static const char what[] = "LZMA encode batch";
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n == 0) return SZ_OK;
  HostBatch<LzmaEncGpuStreamDesc, LzmaEncGpuResult> b;
  SRes r = b.lay_out(
      what, descs, n, src_size, dst_size, workspace_limit,
      [](const LzmaEncGpuStreamDesc& d) { return d.dst_cap; },
      lzmaenc_work, lzmaenc_slice_bytes);
  if (r != SZ_OK) return r;
  const std::vector<LzmaEncGpuStreamDesc> d = in_launch_order(descs, b.plan);
  r = b.queue(what, d, false, src, src_size, one_item ? nullptr : dst, dst_size,
              [&](uint32_t lo, uint32_t cnt) {
                return lzmaencgpu_launch(b.desc.p + lo, nullptr, cnt, b.src.p, b.dst.p, b.ws.p,
                                         b.res.p + lo, LZMA_ENC_GPU_LANES_DEFAULT, nullptr,
                                         lzmaenc_kernels(d.data() + lo, cnt, lzmaenc_check));
              });
  if (r != SZ_OK || (r = b.wait_scattered(what, results)) != SZ_OK) return r;
  const size_t off = one_item ? size_t(descs[0].dst_off) : 0;
  const size_t len =
      one_item ? size_t(std::min<uint64_t>(results[0].dest_len, descs[0].dst_cap)) : dst_size;
  return b.download_dst(dst, off, len) ? SZ_OK : SZ_ERROR_FAIL;
}

extern "C" SRes LzmaEncGpu_EncodeBatchHost(const LzmaEncGpuStreamDesc* descs, size_t n,
                                           const Byte* src, size_t src_size, Byte* dst,
                                           size_t dst_size, LzmaEncGpuResult* results,
                                           uint64_t workspace_limit) {
  return guarded("LZMA encode batch: host allocation failed", [&]() {
    return encode_batch_host(descs, n, src, src_size, dst, dst_size, results, workspace_limit,
                             false);
  });
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
  const char* field = nullptr;
  const int32_t pr =
      lzenc::params_from_props_ex(&e, writeEndMark, lzmaenc_allowed_modes(), &q, &field);
  if (pr == lzenc::kErrParam) return SZ_ERROR_PARAM;
  if (*propsSize < LZMA_PROPS_SIZE) return SZ_ERROR_PARAM;
  if (pr == lzenc::kErrUnsupported) {
    lzmaenc_set_unsupported_error(field);
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
  fill_desc(&d, q);
  LzmaEncGpuResult r;
  r.res = SZ_ERROR_FAIL;
  r.dest_len = 0;
  const SRes res = guarded("LZMA encode: host allocation failed", [&]() {
    return encode_batch_host(&d, 1, src, srcLen, dest, *destLen, &r, 0, true);
  });
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
