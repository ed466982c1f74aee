// lzmaenc_session_capi.hip -- C ABI of the LZMA encoder sessions
// (include/lzma_gpu.h): the host-side planning calls, the round, and the
// LzmaEnc.h handle API (LzmaEnc_Create .. LzmaEnc_MemEncode) as one session fed
// from an ISeqInStream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "host_batch.h"
#include "lzma_gpu_internal.h"
#include "lzmaenc_device.h"
#include "lzmaenc_internal.h"

using namespace lzgpu_host;

static_assert(sizeof(LzmaEncGpuSession) == 200 && offsetof(LzmaEncGpuSession, res) == 104 &&
                  offsetof(LzmaEncGpuSession, low) == 184,
              "session ABI");
static_assert(LZMA_ENC_GPU_SESSION_HOLD == lzenc::kSessionHold &&
                  LZMA_ENC_GPU_SESSION_NEEDS_INPUT == lzenc::kSessionNeedsInput &&
                  LZMA_ENC_GPU_SESSION_FINISHED == lzenc::kSessionFinished &&
                  LZMA_ENC_GPU_SESSION_BUDGET == lzenc::kSessionBudget,
              "session constants");

namespace {

// the props of a session: the fast path whatever the process-wide mask says
int32_t session_params(const CLzmaEncProps* props, int writeEndMark, lzenc::Params* q) {
  lzenc::EncProps e;
  memcpy(&e, props, sizeof(e));
  const char* field = nullptr;
  const int32_t r = lzenc::params_from_props_ex(&e, writeEndMark, 0, q, &field);
  if (r == lzenc::kErrUnsupported)
    set_error((std::string("LZMA encode session: props field ") + (field ? field : "algo") +
               " selects a normal mode (the optimal parser or a bt match finder); sessions are "
               "the fast path alone (levels 0..4: algo 0, btMode 0), whatever the mode mask says")
                  .c_str());
  return r;
}

}  // namespace

extern "C" uint64_t LzmaEncGpu_SessionWorkspaceBytes(const CLzmaEncProps* props,
                                                     uint64_t src_cap) {
  lzenc::Params q;
  if (session_params(props, 0, &q) != lzenc::kOk) return 0;
  if (lzenc::check_params(q, src_cap) != lzenc::kOk) return 0;
  return lzenc::lzmaenc_layout(q, src_cap).bytes;
}

extern "C" SRes LzmaEncGpu_SessionInit(LzmaEncGpuSession* s, const CLzmaEncProps* props,
                                       int writeEndMark, const Byte* d_src, uint64_t src_cap,
                                       Byte* d_dst, uint64_t dst_cap, void* d_workspace,
                                       Byte props5[5]) {
  lzenc::Params q;
  int32_t r = session_params(props, writeEndMark, &q);
  if (r != lzenc::kOk) return r;
  r = lzenc::check_params(q, src_cap);
  if (r == lzenc::kErrUnsupported)
    set_error("LZMA encode session: a source of 2^31 bytes or more is not supported");
  if (r != lzenc::kOk) return r;
  if (reinterpret_cast<uintptr_t>(d_workspace) & 15u) return SZ_ERROR_PARAM;
  lzenc::session_bind(s, q, d_src, src_cap, d_dst, dst_cap, d_workspace);
  lzenc::write_props5(q, props5);
  return SZ_OK;
}

extern "C" size_t LzmaEncGpu_SessionScratchBytes(size_t n) {
  return (size_t(kLzmaEncSessionHeaderWords) + 2 * n) * sizeof(uint32_t);
}

extern "C" SRes LzmaEncGpu_SessionEncodeBatch(LzmaEncGpuSession* d_sessions, size_t n,
                                              void* d_scratch, unsigned lanes, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (lanes != LZMA_ENC_GPU_LANES_DEFAULT && lanes != 16 && lanes != 32 && lanes != 64)
    return SZ_ERROR_PARAM;
  if (n == 0) return SZ_OK;
  if (lzmaencgpu_session_launch(d_sessions, uint32_t(n), static_cast<uint32_t*>(d_scratch), lanes,
                                static_cast<hipStream_t>(stream)) != 0) {
    set_error("LZMA encode session round: kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}

// The list pass alone, for lzmaenc_session_bench.py.
extern "C" SRes LzmaEncGpu_SessionListPass(const LzmaEncGpuSession* d_sessions, size_t n,
                                           void* d_scratch, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  return lzmaencgpu_session_launch_list(d_sessions, uint32_t(n), static_cast<uint32_t*>(d_scratch),
                                        static_cast<hipStream_t>(stream)) == 0
             ? SZ_OK
             : SZ_ERROR_FAIL;
}

// ---------------------------------------------------------------- LzmaEnc.h

namespace {

struct Handle {
  lzenc::EncProps props;  // as SetProps took them (normalised)
};

// what dst needs for a source of n bytes: LzmaLib.h's bound for incompressible
// data (n + n / 3 + 128) and room for the end mark and the flush
uint64_t dst_bound(uint64_t n) { return n + n / 3 + 128 + 16; }

// How LzmaEnc_Encode feeds its session.  Reads are collected on the host until
// kPieceMin bytes wait (or the staging block is full, or the stream ends); they
// are then appended to the device source and one round runs.  The device source
// starts at kSrcStart bytes and doubles when full: a new allocation, one
// device-to-device copy of the stream so far, the old block freed.  dst follows
// (dst_bound of the source's room; the bytes already written out are not
// copied), and so does the slice while the ring is sized by the source
// (src_cap < dictSize): its regions keep their offsets, `son` is last and only
// grows, so the old slice is copied to the front of the new one.
constexpr size_t kPieceMin = size_t(4) << 10, kStage = size_t(1) << 20;
constexpr uint64_t kSrcStart = uint64_t(1) << 20, kSrcMax = (uint64_t(1) << 31) - 1;

struct Feed {
  DevArr<uint8_t> src, dst, ws;
  DevArr<LzmaEncGpuSession> rec;
  DevArr<uint32_t> scratch;
  LzmaEncGpuSession s;
  lzenc::Params q;

  bool grow(uint64_t need) {
    uint64_t cap = s.src_cap ? s.src_cap : kSrcStart;
    while (cap < need) cap = std::min<uint64_t>(cap * 2, kSrcMax);
    if (cap == s.src_cap) return true;
    DevArr<uint8_t> nsrc, ndst, nws;
    const uint64_t ws_bytes = lzenc::lzmaenc_layout(q, cap).bytes;
    const uint64_t old_ws = s.src_cap ? lzenc::lzmaenc_layout(q, s.src_cap).bytes : 0;
    if (!nsrc.alloc(size_t(cap)) || !ndst.alloc(size_t(dst_bound(cap)))) return false;
    if (s.src_len != 0 &&
        !hip_ok(hipMemcpy(nsrc.p, src.p, size_t(s.src_len), hipMemcpyDeviceToDevice), "grow src"))
      return false;
    if (ws_bytes != old_ws) {
      if (!nws.alloc(size_t(ws_bytes))) return false;
      if (old_ws != 0 &&
          !hip_ok(hipMemcpy(nws.p, ws.p, size_t(old_ws), hipMemcpyDeviceToDevice), "grow slice"))
        return false;
      std::swap(ws.p, nws.p);
    }
    std::swap(src.p, nsrc.p);
    std::swap(dst.p, ndst.p);
    s.src = src.p;
    s.dst = dst.p;
    s.ws = ws.p;
    s.src_cap = cap;
    s.dst_cap = dst_bound(cap);
    return true;
  }
};

SRes encode_whole(const lzenc::EncProps& props, ISeqOutStream* outStream, ISeqInStream* inStream,
                  ICompressProgress* progress) {
  std::vector<uint8_t> src;
  for (;;) {
    const size_t at = src.size();
    src.resize(at + kStage);
    size_t got = kStage;
    const SRes rr = inStream->Read(inStream, src.data() + at, &got);
    if (rr != SZ_OK) return rr;
    if (got > kStage) return SZ_ERROR_READ;
    src.resize(at + got);
    if (got == 0) break;
  }
  std::vector<uint8_t> dst(size_t(dst_bound(src.size())));
  SizeT dl = dst.size(), ps = LZMA_PROPS_SIZE;
  Byte props5[LZMA_PROPS_SIZE];
  CLzmaEncProps p;
  memcpy(&p, &props, sizeof(p));
  const SRes r = LzmaEncode(dst.data(), &dl, src.data(), src.size(), &p, props5, &ps,
                            int(props.writeEndMark), nullptr, nullptr, nullptr);
  if (r != SZ_OK) return r;
  if (outStream->Write(outStream, dst.data(), dl) != dl) return SZ_ERROR_WRITE;
  if (progress && progress->Progress(progress, src.size(), dl) != SZ_OK) return SZ_ERROR_PROGRESS;
  return SZ_OK;
}

SRes encode_stream(const Handle* h, ISeqOutStream* outStream, ISeqInStream* inStream,
                   ICompressProgress* progress) {
  // LzmaEnc_SetProps' verdict, then what this library does not encode
  lzenc::Params q;
  const char* field = nullptr;
  const int32_t pr = lzenc::params_from_props_ex(&h->props, int(h->props.writeEndMark),
                                                 lzmaenc_allowed_modes(), &q, &field);
  if (pr == lzenc::kErrUnsupported) lzmaenc_set_unsupported_error(field);
  if (pr != lzenc::kOk) return pr;
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (lzenc::mode_of(q) != 0) return encode_whole(h->props, outStream, inStream, progress);

  Feed f;
  f.q = q;
  lzenc::session_bind(&f.s, q, nullptr, 0, nullptr, 0, nullptr);
  if (!f.rec.alloc(1) || !f.scratch.alloc(LzmaEncGpu_SessionScratchBytes(1) / 4) ||
      !f.grow(kSrcStart)) {
    set_error("LZMA encode: device allocation failed");
    return SZ_ERROR_MEM;
  }
  std::vector<uint8_t> stage(kStage), out;
  size_t staged = 0;
  uint64_t written = 0;
  bool eof = false;
  while (!f.s.finished) {
    while (!eof && staged < kStage) {
      size_t got = kStage - staged;
      const SRes rr = inStream->Read(inStream, stage.data() + staged, &got);
      if (rr != SZ_OK) return rr;
      if (got > kStage - staged) return SZ_ERROR_READ;
      if (got == 0) eof = true;
      staged += got;
      if (staged >= kPieceMin) break;
    }
    if (f.s.src_len + staged > kSrcMax) {
      set_error("LZMA encode: a source of 2^31 bytes or more is not supported");
      return SZ_ERROR_UNSUPPORTED;
    }
    if (!f.grow(f.s.src_len + staged)) {
      set_error("LZMA encode: device allocation failed");
      return SZ_ERROR_MEM;
    }
    if (staged != 0 && !hip_ok(hipMemcpy(f.src.p + f.s.src_len, stage.data(), staged,
                                         hipMemcpyHostToDevice), "upload piece"))
      return SZ_ERROR_FAIL;
    f.s.src_len += staged;
    staged = 0;
    f.s.finish = eof ? 1u : 0u;
    f.s.in_budget = 0;
    if (!hip_ok(hipMemcpy(f.rec.p, &f.s, sizeof(f.s), hipMemcpyHostToDevice), "upload session"))
      return SZ_ERROR_FAIL;
    if (lzmaencgpu_session_launch(f.rec.p, 1, f.scratch.p, LZMA_ENC_GPU_LANES_DEFAULT, nullptr) !=
        0) {
      set_error("LZMA encode session round: kernel launch failed");
      return SZ_ERROR_FAIL;
    }
    if (!hip_ok(hipMemcpy(&f.s, f.rec.p, sizeof(f.s), hipMemcpyDeviceToHost), "session round"))
      return SZ_ERROR_FAIL;
    const uint64_t upto = std::min<uint64_t>(f.s.out_pos, f.s.dst_cap);
    if (upto > written) {
      out.resize(size_t(upto - written));
      if (!hip_ok(hipMemcpy(out.data(), f.dst.p + written, out.size(), hipMemcpyDeviceToHost),
                  "download piece"))
        return SZ_ERROR_FAIL;
      if (outStream->Write(outStream, out.data(), out.size()) != out.size()) return SZ_ERROR_WRITE;
      written = upto;
    }
    if (progress && progress->Progress(progress, f.s.in_pos, f.s.out_pos) != SZ_OK)
      return SZ_ERROR_PROGRESS;
  }
  return f.s.res;
}

}  // namespace

extern "C" CLzmaEncHandle LzmaEnc_Create(ISzAlloc* alloc) {
  Handle* h = static_cast<Handle*>(alloc->Alloc(alloc, sizeof(Handle)));
  if (!h) return nullptr;
  lzenc::props_init(&h->props);
  lzenc::props_normalize(&h->props);
  return h;
}

extern "C" void LzmaEnc_Destroy(CLzmaEncHandle p, ISzAlloc* alloc, ISzAlloc* allocBig) {
  (void)allocBig;
  alloc->Free(alloc, p);
}

// LzmaEnc_SetProps (LzmaEnc.c:391-443): its checks; what the modes mask refuses
// is decided when the handle encodes, as the mask may change until then
extern "C" SRes LzmaEnc_SetProps(CLzmaEncHandle p, const CLzmaEncProps* props2) {
  Handle* h = static_cast<Handle*>(p);
  lzenc::EncProps e;
  memcpy(&e, props2, sizeof(e));
  lzenc::props_normalize(&e);
  if (e.lc > 8 || e.lp > 4 || e.pb > 4 || e.dictSize > lzenc::kDictMax) return SZ_ERROR_PARAM;
  h->props = e;
  return SZ_OK;
}

extern "C" SRes LzmaEnc_WriteProperties(CLzmaEncHandle p, Byte* properties, SizeT* size) {
  const Handle* h = static_cast<const Handle*>(p);
  if (*size < LZMA_PROPS_SIZE) return SZ_ERROR_PARAM;
  lzenc::Params q;
  const int32_t r = lzenc::params_from_props_ex(&h->props, 0, 3, &q);
  if (r == lzenc::kErrUnsupported) {  // Bt2 / Bt3: the header bytes need no finder
    lzenc::EncProps e = h->props;
    e.btMode = 0;
    if (lzenc::params_from_props_ex(&e, 0, 3, &q) != lzenc::kOk) return SZ_ERROR_PARAM;
  } else if (r != lzenc::kOk) {
    return r;
  }
  *size = LZMA_PROPS_SIZE;
  lzenc::write_props5(q, properties);
  return SZ_OK;
}

extern "C" SRes LzmaEnc_Encode(CLzmaEncHandle p, ISeqOutStream* outStream, ISeqInStream* inStream,
                               ICompressProgress* progress, ISzAlloc* alloc, ISzAlloc* allocBig) {
  (void)alloc;
  (void)allocBig;
  const Handle* h = static_cast<const Handle*>(p);
  return guarded("LZMA encode: host allocation failed",
                 [&]() { return encode_stream(h, outStream, inStream, progress); });
}

extern "C" SRes LzmaEnc_MemEncode(CLzmaEncHandle p, Byte* dest, SizeT* destLen, const Byte* src,
                                  SizeT srcLen, int writeEndMark, ICompressProgress* progress,
                                  ISzAlloc* alloc, ISzAlloc* allocBig) {
  const Handle* h = static_cast<const Handle*>(p);
  CLzmaEncProps props;
  memcpy(&props, &h->props, sizeof(props));
  Byte props5[LZMA_PROPS_SIZE];
  SizeT ps = LZMA_PROPS_SIZE;
  return LzmaEncode(dest, destLen, src, srcLen, &props, props5, &ps, writeEndMark, progress, alloc,
                    allocBig);
}
