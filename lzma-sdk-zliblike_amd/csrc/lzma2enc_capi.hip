// lzma2enc_capi.hip -- C ABI of the LZMA2 and xz writers (include/lzma_gpu.h):
// the CLzma2EncProps drop-ins, block planning, the device and host batch
// calls, the compaction, one host buffer as one LZMA2 stream or one xz stream,
// and Lzma2Enc_Create / SetProps / WriteProperties / Encode over those.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string.h>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "host_batch.h"
#include "lzma2enc_device.h"
#include "lzma2enc_internal.h"
#include "lzma_gpu_internal.h"

using namespace lzgpu_host;

static_assert(sizeof(CLzma2EncProps) == 64 && sizeof(lzenc::Enc2Props) == sizeof(CLzma2EncProps) &&
                  offsetof(CLzma2EncProps, blockSize) == 48,
              "CLzma2EncProps layout (Lzma2Enc.h:13-19)");

static lzenc::Enc2Props to_enc2(const CLzma2EncProps* p) {
  lzenc::Enc2Props e;
  memcpy(&e, p, sizeof(e));
  return e;
}

extern "C" void Lzma2EncProps_Init(CLzma2EncProps* p) {
  lzenc::Enc2Props e;
  lzenc::props2_init(&e);
  memcpy(p, &e, sizeof(e));
}

extern "C" void Lzma2EncProps_Normalize(CLzma2EncProps* p) {
  lzenc::Enc2Props e = to_enc2(p);
  lzenc::props2_normalize(&e);
  memcpy(p, &e, sizeof(e));
}

extern "C" size_t Lzma2EncGpu_BlockBound(size_t src_len) {
  return src_len + (src_len >> 10) + 16;
}

static void fill_desc(LzmaEncGpuStreamDesc* desc, const lzenc::Params& q) {
  desc->dict_size = q.dict_size;
  desc->lc = q.lc;
  desc->lp = q.lp;
  desc->pb = q.pb;
  desc->fb = q.fb;
  desc->mc = q.mc;
  desc->write_end_mark = 0;
  desc->mode = lzenc::mode_of(q);
}

// lzma2_params_from_props_ex with the refusal put into the last error
static int32_t params_of(const lzenc::Enc2Props* e, uint32_t allowed, lzenc::Params* q,
                         uint8_t* prop) {
  const char* field = nullptr;
  const int32_t r = lzenc::lzma2_params_from_props_ex(e, allowed, q, prop, &field);
  if (r == lzenc::kErrUnsupported) lzmaenc_set_unsupported_error(field);
  return r;
}

extern "C" SRes Lzma2EncGpu_DescFromPropsEx(const CLzma2EncProps* props, unsigned allowed,
                                            LzmaEncGpuStreamDesc* desc, Byte* prop) {
  const lzenc::Enc2Props e = to_enc2(props);
  lzenc::Params q;
  uint8_t pr = 0;
  const int32_t r = params_of(&e, allowed, &q, &pr);
  if (r != lzenc::kOk) return r;
  fill_desc(desc, q);
  *prop = pr;
  return SZ_OK;
}

extern "C" SRes Lzma2EncGpu_DescFromProps(const CLzma2EncProps* props, LzmaEncGpuStreamDesc* desc,
                                          Byte* prop) {
  return Lzma2EncGpu_DescFromPropsEx(props, lzmaenc_allowed_modes(), desc, prop);
}

extern "C" SRes Lzma2EncGpu_PlanBatch(LzmaEncGpuStreamDesc* descs, size_t n, uint32_t* order,
                                      uint64_t* workspace_bytes) {
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  return guarded("LZMA2 encode plan: host allocation failed", [&]() -> SRes {
    uint64_t at = 0;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t need = lzma2enc_slice_bytes(descs[i]);
      descs[i].ws_off = need ? at : 0;
      at += need;
    }
    if (workspace_bytes) *workspace_bytes = at;
    if (order) longest_first(n, [&](uint32_t i) { return lzmaenc_work(descs[i]); }, order);
    return SZ_OK;
  });
}

extern "C" SRes Lzma2EncGpu_EncodeBatch(const LzmaEncGpuStreamDesc* d_descs,
                                        const uint32_t* d_order, size_t n, const Byte* d_src,
                                        Byte* d_dst, void* d_workspace,
                                        LzmaEncGpuResult* d_results, unsigned lanes,
                                        void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (lanes != LZMA_ENC_GPU_LANES_DEFAULT && lanes != 16 && lanes != 32 && lanes != 64)
    return SZ_ERROR_PARAM;
  if (n == 0) return SZ_OK;
  if (lzma2encgpu_launch(d_descs, d_order, 0, uint32_t(n), uint32_t(n), d_src, d_dst,
                         static_cast<uint8_t*>(d_workspace), d_results, lanes,
                         static_cast<hipStream_t>(stream)) != 0) {
    set_error("LZMA2 encode batch kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

extern "C" SRes Lzma2EncGpu_Compact(const LzmaEncGpuStreamDesc* d_descs,
                                    const LzmaEncGpuResult* d_results, size_t n,
                                    const Byte* d_slots, Byte* d_out, uint64_t out_cap,
                                    uint64_t* d_offsets, LzmaEncGpuResult* d_total, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (lzma2encgpu_launch_compact(d_descs, d_results, uint32_t(n), d_slots, d_out, out_cap,
                                 d_offsets, d_total, static_cast<hipStream_t>(stream)) != 0) {
    set_error("LZMA2 compaction kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

namespace {

// The device side of one host call: the source, the blocks' slots, the
// descriptors and results in the caller's index order, the launch order.
typedef HostBatch<LzmaEncGpuStreamDesc, LzmaEncGpuResult> Batch;

// Uploads src (and dst when dst_init is given), lays the workspace out over
// the longest-first order in as many launches as keep it at or under the
// limit, and queues them on the null stream; before(): what is queued between
// the uploads and the first launch (0 on success).  The caller synchronises.
template <class Before>
SRes run_batch(const LzmaEncGpuStreamDesc* descs, size_t n, const Byte* src, size_t src_size,
               const Byte* dst_init, size_t dst_size, uint64_t workspace_limit, Batch& b,
               Before before) {
  static const char what[] = "LZMA2 encode batch";
  const SRes r = b.lay_out(
      what, descs, n, src_size, dst_size, workspace_limit,
      [](const LzmaEncGpuStreamDesc& d) { return d.dst_cap; },
      lzmaenc_work, lzma2enc_slice_bytes);
  if (r != SZ_OK) return r;
  // over the descriptors the device sees: the caller's ws_off is not looked at
  const std::vector<LzmaEncGpuStreamDesc> d = in_caller_order(descs, b.plan);
  const uint32_t kernels = lzmaenc_kernels(d.data(), n, lzma2enc_check);
  bool first = true;
  return b.queue(what, d, true, src, src_size, dst_init, dst_size,
                 [&](uint32_t lo, uint32_t cnt) {
                   if (first && before() != 0) return -1;
                   first = false;
                   return lzma2encgpu_launch(b.desc.p, b.order.p, lo, cnt, uint32_t(n), b.src.p,
                                             b.dst.p, b.ws.p, b.res.p, LZMA_ENC_GPU_LANES_DEFAULT,
                                             nullptr, kernels);
                 });
}

// Lzma2Enc_SetProps' and LzmaEnc_SetProps' verdict on the props, the
// normalised props and the encoder's parameters
SRes resolve_props(const CLzma2EncProps* props, lzenc::Enc2Props* norm, lzenc::Params* q,
                   Byte* prop) {
  const lzenc::Enc2Props e = to_enc2(props);
  uint8_t pr = 0;
  const int32_t r = params_of(&e, lzmaenc_allowed_modes(), q, &pr);
  if (r != lzenc::kOk) return r;
  *norm = e;
  lzenc::props2_normalize(norm);
  if (prop) *prop = pr;
  return SZ_OK;
}

// src cut into block_size pieces, each with a slot of its bound
SRes cut_blocks(size_t src_len, size_t block_size, const lzenc::Params& q,
                std::vector<LzmaEncGpuStreamDesc>& descs, uint64_t* slots_bytes) {
  if (block_size == 0) return SZ_ERROR_PARAM;
  if (block_size > src_len) block_size = src_len ? src_len : 1;
  if (block_size >= (uint64_t(1) << 31)) {
    set_error("LZMA2 encode: one block of 2^31 bytes or more is not supported");
    return SZ_ERROR_UNSUPPORTED;
  }
  const uint64_t n = (uint64_t(src_len) + block_size - 1) / block_size;
  if (n > 0x7FFFFFFFull) {
    set_error("LZMA2 encode: 2^31 blocks or more");
    return SZ_ERROR_UNSUPPORTED;
  }
  descs.resize(size_t(n));
  uint64_t at = 0;
  for (size_t i = 0; i < n; ++i) {
    LzmaEncGpuStreamDesc& d = descs[i];
    memset(&d, 0, sizeof(d));
    fill_desc(&d, q);
    d.src_off = uint64_t(i) * block_size;
    d.src_len = std::min<uint64_t>(block_size, src_len - d.src_off);
    d.dst_off = at;
    d.dst_cap = Lzma2EncGpu_BlockBound(size_t(d.src_len));
    at += d.dst_cap;
  }
  *slots_bytes = at;
  return SZ_OK;
}

// What one host buffer's encode leaves on the host: the compacted stream
// (chunks of every block, then 0x00) and where each block starts in it.
struct Stream {
  std::vector<uint8_t> bytes;
  std::vector<uint64_t> offsets;  // n + 1
  std::vector<LzmaEncGpuStreamDesc> descs;
  Batch b;
  // with a filter chain: b.src is filtered in place before the encode, `plain`
  // keeps the source as uploaded for the block checks
  DevArr<uint8_t> plain;
  FilterJob filter_jobs[LZMA_GPU_XZ_ENC_FILTERS_MAX];
  const Byte* check_src() const { return plain.p ? plain.p : b.src.p; }
};

// The chain over every block of the uploaded source, first filter first in the
// encode direction, one batch per filter; every block starts from a fresh state
// at ip = the start offset.
SRes queue_chain(Stream& s, size_t src_len, const LzmaGpuXzFilter* filters, unsigned num_filters) {
  static const char what[] = "xz encode filters";
  const size_t n = s.descs.size();
  const SRes ar = alloc_all(what, s.plain, src_len);
  if (ar != SZ_OK) return ar;
  if (!hip_ok(hipMemcpyAsync(s.plain.p, s.b.src.p, src_len, hipMemcpyDeviceToDevice, nullptr),
              what))
    return SZ_ERROR_FAIL;
  std::vector<uint64_t> off(n), len(n);
  for (size_t i = 0; i < n; ++i) {
    off[i] = s.descs[i].src_off;
    len[i] = s.descs[i].src_len;
  }
  for (unsigned k = 0; k < num_filters; ++k) {
    const std::vector<uint32_t> prop(n, filters[k].prop);
    const SRes r =
        queue_filter(what, s.filter_jobs[k], filters[k].id, s.b.src.p, off, len, prop.data(), 1);
    if (r != SZ_OK) return r;
  }
  return SZ_OK;
}

// upload, one batch, compaction, download of offsets and stream
SRes encode_stream(const Byte* src, size_t src_len, size_t block_size, const lzenc::Params& q,
                   Stream& s, const LzmaGpuXzFilter* filters = nullptr,
                   unsigned num_filters = 0) {
  uint64_t slots_bytes = 0;
  const SRes cr = cut_blocks(src_len, block_size, q, s.descs, &slots_bytes);
  if (cr != SZ_OK) return cr;
  if (!ensure_device()) return SZ_ERROR_FAIL;
  const size_t n = s.descs.size();
  SRes chain = SZ_OK;
  const SRes rr = run_batch(s.descs.data(), n, src, src_len, nullptr, size_t(slots_bytes), 0, s.b,
                            [&] {
                              if (num_filters) chain = queue_chain(s, src_len, filters, num_filters);
                              return chain == SZ_OK ? 0 : -1;
                            });
  if (chain != SZ_OK) return chain;
  if (rr != SZ_OK) return rr;
  DevArr<uint8_t> g_out;
  DevArr<uint64_t> g_off;
  DevArr<LzmaEncGpuResult> g_total;
  const uint64_t out_cap = slots_bytes + 1;
  const SRes ar = alloc_all("LZMA2 encode", g_out, size_t(out_cap), g_off, n + 1, g_total, 1);
  if (ar != SZ_OK) return ar;
  if (lzma2encgpu_launch_compact(s.b.desc.p, s.b.res.p, uint32_t(n), s.b.dst.p, g_out.p, out_cap,
                                 g_off.p, g_total.p, nullptr) != 0) {
    set_error("LZMA2 compaction kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  LzmaEncGpuResult total;
  s.offsets.resize(n + 1);
  if (!hip_ok(hipDeviceSynchronize(), "LZMA2 encode") ||
      !hip_ok(hipMemcpy(&total, g_total.p, sizeof(total), hipMemcpyDeviceToHost),
              "download total") ||
      !hip_ok(hipMemcpy(s.offsets.data(), g_off.p, (n + 1) * sizeof(uint64_t),
                        hipMemcpyDeviceToHost), "download offsets"))
    return SZ_ERROR_FAIL;
  if (total.res != SZ_OK) {  // a slot of the block bound always fits its block
    set_error("LZMA2 encode: a block failed on the device");
    return total.res == SZ_ERROR_OUTPUT_EOF ? SZ_ERROR_FAIL : total.res;
  }
  s.bytes.resize(size_t(total.dest_len));
  if (!hip_ok(hipMemcpy(s.bytes.data(), g_out.p, s.bytes.size(), hipMemcpyDeviceToHost),
              "download stream"))
    return SZ_ERROR_FAIL;
  return SZ_OK;
}

struct Handle {
  ISzAlloc* alloc;
  lzenc::Enc2Props props;  // as given to SetProps, normalised
};

void put32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = uint8_t(v >> (8 * i));
}
void put_varint(std::vector<uint8_t>& out, uint64_t v) {
  while (v >= 0x80) {
    out.push_back(uint8_t(v | 0x80));
    v >>= 7;
  }
  out.push_back(uint8_t(v));
}

// the block checks of an xz stream, on the device over the uploaded source
SRes block_checks(const Stream& s, unsigned check_size, std::vector<uint8_t>& checks) {
  const size_t n = s.descs.size();
  checks.assign(n * check_size, 0);
  if (check_size == 0 || n == 0) return SZ_OK;
  std::vector<uint64_t> off(n), len(n);
  for (size_t i = 0; i < n; ++i) {
    off[i] = s.descs[i].src_off;
    len[i] = s.descs[i].src_len;
  }
  RangeChecks k;
  SRes r = k.prepare("xz encode", check_size, off, len);
  if (r != SZ_OK || (r = k.launch(s.check_src())) != SZ_OK) return r;
  if (!hip_ok(hipDeviceSynchronize(), "xz block checks") ||
      !k.fetch(checks.data(), "download checks"))
    return SZ_ERROR_FAIL;
  return SZ_OK;
}

// the reader's rules for a chain (xz_capi.hip, BraState_SetProps XzDec.c:71-109)
SRes check_chain(const LzmaGpuXzFilter* filters, unsigned num_filters) {
  if (num_filters > LZMA_GPU_XZ_ENC_FILTERS_MAX) return SZ_ERROR_PARAM;
  for (unsigned k = 0; k < num_filters; ++k) {
    const uint32_t id = filters[k].id, prop = filters[k].prop;
    if (id == 3) {
      if (prop < 1 || prop > 256) return SZ_ERROR_PARAM;
    } else if (id >= 4 && id <= 9) {
      const uint32_t align = id == 6 ? 0xF : (id == 8 ? 1 : (id == 4 ? 0 : 3));
      if (prop & align) return SZ_ERROR_PARAM;
    } else {
      set_error("xz encode: only delta and the branch converters (ids 3..9) are written");
      return SZ_ERROR_UNSUPPORTED;
    }
  }
  return SZ_OK;
}

SRes xz_encode(Byte* dest, SizeT* destLen, const Byte* src, SizeT srcLen,
               const CLzma2EncProps* props, unsigned check_type, const LzmaGpuXzFilter* filters,
               unsigned num_filters) {
  const SRes cr = check_chain(filters, num_filters);
  if (cr != SZ_OK) return cr;
  unsigned check_size;
  switch (check_type) {
    case LZMA_GPU_XZ_CHECK_NONE: check_size = 0; break;
    case LZMA_GPU_XZ_CHECK_CRC32: check_size = 4; break;
    case LZMA_GPU_XZ_CHECK_CRC64: check_size = 8; break;
    case LZMA_GPU_XZ_CHECK_SHA256: check_size = 32; break;
    default:
      set_error("xz encode: only the checks none, CRC-32, CRC-64 and SHA-256 are written");
      return SZ_ERROR_UNSUPPORTED;
  }
  lzenc::Enc2Props norm;
  lzenc::Params q;
  Byte prop = 0;
  const SRes pr = resolve_props(props, &norm, &q, &prop);
  if (pr != SZ_OK) return pr;
  if (!ensure_device()) return SZ_ERROR_FAIL;
  Stream s;
  std::vector<uint8_t> checks;
  if (srcLen != 0) {
    const SRes er = encode_stream(src, srcLen, norm.blockSize, q, s, filters, num_filters);
    if (er != SZ_OK) return er;
    const SRes kr = block_checks(s, check_size, checks);
    if (kr != SZ_OK) return kr;
  }
  const size_t n = s.descs.size();
  // Xz_WriteHeader, XzBlock_WriteHeader (no size fields; the chain, then LZMA2),
  // Xz_WriteFooter
  const uint8_t flags[2] = {0, uint8_t(check_type)};
  std::vector<uint8_t> bh{0, uint8_t(num_filters)};
  for (unsigned k = 0; k < num_filters; ++k) {
    bh.push_back(uint8_t(filters[k].id));
    if (filters[k].id == 3) {
      bh.push_back(1);
      bh.push_back(uint8_t(filters[k].prop - 1));
    } else if (filters[k].prop == 0) {
      bh.push_back(0);
    } else {
      bh.push_back(4);
      for (int i = 0; i < 4; ++i) bh.push_back(uint8_t(filters[k].prop >> (8 * i)));
    }
  }
  bh.push_back(0x21);
  bh.push_back(1);
  bh.push_back(prop);
  while (bh.size() & 3) bh.push_back(0);
  bh[0] = uint8_t(bh.size() / 4);  // the size with the CRC, in words, less one
  bh.resize(bh.size() + 4);
  put32(bh.data() + bh.size() - 4, crc32_host(bh.data(), bh.size() - 4));
  std::vector<uint8_t> index{0};
  put_varint(index, n);
  uint64_t total = 12;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t pack = s.offsets[i + 1] - s.offsets[i] + 1;  // the chunks and 0x00
    put_varint(index, bh.size() + pack + check_size);
    put_varint(index, s.descs[i].src_len);
    total += bh.size() + ((pack + 3) & ~uint64_t(3)) + check_size;
  }
  while (index.size() & 3) index.push_back(0);
  index.resize(index.size() + 4);
  put32(index.data() + index.size() - 4, crc32_host(index.data(), index.size() - 4));
  total += index.size() + 12;
  if (total > *destLen) {
    *destLen = 0;
    return SZ_ERROR_OUTPUT_EOF;
  }
  uint8_t* p = dest;
  memcpy(p, "\xFD" "7zXZ\0", 6);
  memcpy(p + 6, flags, 2);
  put32(p + 8, crc32_host(flags, 2));
  p += 12;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t len = s.offsets[i + 1] - s.offsets[i];
    memcpy(p, bh.data(), bh.size());
    p += bh.size();
    memcpy(p, s.bytes.data() + s.offsets[i], size_t(len));
    p += len;
    *p++ = 0;
    for (uint64_t k = len + 1; k & 3; ++k) *p++ = 0;
    memcpy(p, checks.data() + i * check_size, check_size);
    p += check_size;
  }
  memcpy(p, index.data(), index.size());
  p += index.size();
  put32(p + 4, uint32_t(index.size() / 4 - 1));
  memcpy(p + 8, flags, 2);
  put32(p, crc32_host(p + 4, 6));
  p[10] = 'Y';
  p[11] = 'Z';
  p += 12;
  *destLen = SizeT(p - dest);
  return SZ_OK;
}

SRes lzma2_encode_host(Byte* dest, SizeT* destLen, const Byte* src, SizeT srcLen,
                       const CLzma2EncProps* props, Byte* prop) {
  lzenc::Enc2Props norm;
  lzenc::Params q;
  const SRes pr = resolve_props(props, &norm, &q, prop);
  if (pr != SZ_OK) return pr;
  if (!ensure_device()) return SZ_ERROR_FAIL;
  Stream s;
  if (srcLen == 0) {
    s.bytes.assign(1, 0);
  } else {
    const SRes er = encode_stream(src, srcLen, norm.blockSize, q, s);
    if (er != SZ_OK) return er;
  }
  if (s.bytes.size() > *destLen) {
    *destLen = 0;
    return SZ_ERROR_OUTPUT_EOF;
  }
  memcpy(dest, s.bytes.data(), s.bytes.size());
  *destLen = s.bytes.size();
  return SZ_OK;
}

SRes lzma2enc_encode(Handle* h, ISeqOutStream* outStream, ISeqInStream* inStream,
                     ICompressProgress* progress) {
  // Lzma2EncInt_Init's LzmaEnc_SetProps, then what this library does not encode
  lzenc::Params q;
  uint8_t prop;
  const int32_t pr = params_of(&h->props, lzmaenc_allowed_modes(), &q, &prop);
  if (pr != lzenc::kOk) return pr;
  if (!ensure_device()) return SZ_ERROR_FAIL;
  std::vector<uint8_t> src;
  for (;;) {
    const size_t at = src.size(), step = size_t(1) << 20;
    src.resize(at + step);
    size_t got = step;
    if (inStream->Read(inStream, src.data() + at, &got) != SZ_OK) return SZ_ERROR_READ;
    if (got > step) return SZ_ERROR_READ;
    src.resize(at + got);
    if (got == 0) break;
  }
  if (src.size() >= (uint64_t(1) << 31) && h->props.numBlockThreads <= 1) {
    set_error("LZMA2 encode: one block of 2^31 bytes or more is not supported");
    return SZ_ERROR_UNSUPPORTED;
  }
  Stream s;
  if (!src.empty()) {
    // numBlockThreads <= 1: Lzma2Enc_EncodeMt1, the whole input is one block
    const size_t block = h->props.numBlockThreads <= 1 ? src.size() : h->props.blockSize;
    const SRes er = encode_stream(src.data(), src.size(), block, q, s);
    if (er != SZ_OK) return er;
  } else {
    s.bytes.assign(1, 0);
    s.offsets.assign(1, 0);
  }
  const size_t n = s.descs.size();
  uint64_t in_done = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t len = size_t(s.offsets[i + 1] - s.offsets[i]);
    if (outStream->Write(outStream, s.bytes.data() + s.offsets[i], len) != len)
      return SZ_ERROR_WRITE;
    in_done += s.descs[i].src_len;
    if (progress && progress->Progress(progress, in_done, s.offsets[i + 1]) != SZ_OK)
      return SZ_ERROR_PROGRESS;
  }
  const Byte zero = 0;
  if (outStream->Write(outStream, &zero, 1) != 1) return SZ_ERROR_WRITE;
  return SZ_OK;
}

}  // namespace

extern "C" SRes Lzma2EncGpu_EncodeBatchHost(const LzmaEncGpuStreamDesc* descs, size_t n,
                                            const Byte* src, size_t src_size, Byte* dst,
                                            size_t dst_size, LzmaEncGpuResult* results,
                                            uint64_t workspace_limit) {
  return guarded("LZMA2 encode batch: host allocation failed", [&]() -> SRes {
    if (!ensure_device()) return SZ_ERROR_FAIL;
    if (n == 0) return SZ_OK;
    Batch b;
    SRes r = run_batch(descs, n, src, src_size, dst, dst_size, workspace_limit, b,
                       [] { return 0; });
    if (r != SZ_OK || (r = b.wait("LZMA2 encode batch", results, n)) != SZ_OK) return r;
    return b.download_dst(dst, 0, dst_size) ? SZ_OK : SZ_ERROR_FAIL;
  });
}

extern "C" SRes LzmaGpu_Lzma2EncodeHost(Byte* dest, SizeT* destLen, const Byte* src, SizeT srcLen,
                                        const CLzma2EncProps* props, Byte* prop) {
  return guarded("LZMA2 encode: host allocation failed",
                 [&]() { return lzma2_encode_host(dest, destLen, src, srcLen, props, prop); });
}

extern "C" SRes LzmaGpu_XzEncode(Byte* dest, SizeT* destLen, const Byte* src, SizeT srcLen,
                                 const CLzma2EncProps* props, unsigned check_type) {
  return LzmaGpu_XzEncodeEx(dest, destLen, src, srcLen, props, check_type, nullptr, 0);
}

extern "C" SRes LzmaGpu_XzEncodeEx(Byte* dest, SizeT* destLen, const Byte* src, SizeT srcLen,
                                   const CLzma2EncProps* props, unsigned check_type,
                                   const LzmaGpuXzFilter* filters, unsigned num_filters) {
  return guarded("xz encode: host allocation failed", [&]() {
    return xz_encode(dest, destLen, src, srcLen, props, check_type, filters, num_filters);
  });
}

extern "C" CLzma2EncHandle Lzma2Enc_Create(ISzAlloc* alloc, ISzAlloc* allocBig) {
  (void)allocBig;
  Handle* h = static_cast<Handle*>(alloc->Alloc(alloc, sizeof(Handle)));
  if (!h) return nullptr;
  h->alloc = alloc;
  lzenc::props2_init(&h->props);
  lzenc::props2_normalize(&h->props);
  return h;
}

extern "C" void Lzma2Enc_Destroy(CLzma2EncHandle pp) {
  Handle* h = static_cast<Handle*>(pp);
  h->alloc->Free(h->alloc, h);
}

extern "C" SRes Lzma2Enc_SetProps(CLzma2EncHandle pp, const CLzma2EncProps* props) {
  Handle* h = static_cast<Handle*>(pp);
  lzenc::Enc2Props e = to_enc2(props);
  lzenc::EncProps lzmaProps = e.lzmaProps;
  lzenc::props_normalize(&lzmaProps);
  if (lzmaProps.lc + lzmaProps.lp > int(lzenc::kLzma2LcLpMax)) return SZ_ERROR_PARAM;
  lzenc::props2_normalize(&e);
  h->props = e;
  return SZ_OK;
}

extern "C" Byte Lzma2Enc_WriteProperties(CLzma2EncHandle pp) {
  const Handle* h = static_cast<const Handle*>(pp);
  lzenc::EncProps lzmaProps = h->props.lzmaProps;
  lzenc::props_normalize(&lzmaProps);
  return lzenc::lzma2_prop_byte(lzmaProps.dictSize);
}

extern "C" SRes Lzma2Enc_Encode(CLzma2EncHandle pp, ISeqOutStream* outStream,
                                ISeqInStream* inStream, ICompressProgress* progress) {
  Handle* h = static_cast<Handle*>(pp);
  return guarded("LZMA2 encode: host allocation failed",
                 [&]() { return lzma2enc_encode(h, outStream, inStream, progress); });
}
