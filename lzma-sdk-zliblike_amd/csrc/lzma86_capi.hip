// lzma86_capi.hip -- C ABI of the Lzma86 batch (include/lzma_gpu.h; Lzma86.h,
// Lzma86Enc.c, Lzma86Dec.c): per-stream checks and the candidates' descriptors,
// the scratch layout, the device and host batch calls in both directions, and
// Lzma86_Encode / Lzma86_GetUnpackSize / Lzma86_Decode as one-item calls of the
// host forms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <string.h>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "host_batch.h"
#include "lzma86_device.h"
#include "lzma86_internal.h"
#include "lzma_gpu_internal.h"
#include "lzmaenc_device.h"
#include "lzmaenc_internal.h"

using namespace lzgpu_host;

static_assert(sizeof(Lzma86GpuStreamDesc) == 48 && sizeof(Lzma86GpuResult) == 24 &&
                  sizeof(Lzma86GpuStats) == 64,
              "Lzma86 ABI");
static_assert(sizeof(lz86::Stream) == 64 && sizeof(lz86::StageJob) == 24 &&
                  sizeof(lz86::DecStream) == 16,
              "Lzma86 device tables");
static_assert(LZMA86_HEADER_SIZE == lz86::kHeader, "Lzma86.h:12");

namespace {

typedef HostBatch<Lzma86GpuStreamDesc, Lzma86GpuResult> Batch;

constexpr uint64_t kTableAlign = 256;
uint64_t up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

uint64_t now_ns() {
  return uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(
                      std::chrono::steady_clock::now().time_since_epoch())
                      .count());
}

// a table's place in the scratch
struct Place {
  uint64_t at = 0, total = 0;
  uint64_t take(uint64_t bytes) {
    const uint64_t o = total;
    total = up(total + bytes, kTableAlign);
    return o;
  }
};

// ---------------------------------------------------------------- encode

struct EncJob {
  size_t n = 0;
  std::vector<lz86::Stream> streams;        // caller order
  std::vector<LzmaEncGpuStreamDesc> tmpl;   // a stream's candidate without its places
  std::vector<uint64_t> slice;              // one candidate's workspace slice
  std::vector<uint8_t> has_u, has_f;
  std::vector<uint64_t> src_off;            // stream -> its source in d_src
  LaunchPlan plan;                          // over the streams
  std::vector<size_t> cand_start;           // plan position -> first candidate, n + 1 entries
  std::vector<uint64_t> filt_off;           // stream -> its copy in the filter area
  std::vector<lz86::StageJob> stage;
  std::vector<uint32_t> large;
  uint64_t filt_bytes = 0, slots_bytes = 0, max_stage = 0, max_large = 0;
  uint64_t o_streams = 0, o_cands = 0, o_cres = 0, o_stage = 0, o_r64 = 0, o_r32 = 0, o_large = 0,
           o_filt = 0, o_slots = 0, o_ws = 0, total = 0;
  size_t candidates() const { return cand_start.empty() ? 0 : cand_start.back(); }
  uint32_t n_cand(size_t i) const { return uint32_t(has_u[i]) + uint32_t(has_f[i]); }
};

// Lzma86_Encode's checks before the first pass, then LzmaEncode's on the props
// and what this library does not encode
void enc_streams(const Lzma86GpuStreamDesc* descs, size_t n, EncJob& j) {
  j.n = n;
  j.streams.resize(n);
  j.tmpl.resize(n);
  j.slice.assign(n, 0);
  j.has_u.assign(n, 0);
  j.has_f.assign(n, 0);
  j.src_off.resize(n);
  const uint32_t allowed = lzmaenc_allowed_modes();
  for (size_t i = 0; i < n; ++i) {
    const Lzma86GpuStreamDesc& d = descs[i];
    lz86::Stream& s = j.streams[i];
    memset(&s, 0, sizeof(s));
    s.dst_off = d.dst_off;
    s.dst_cap = d.dst_cap;
    s.src_len = d.src_len;
    j.src_off[i] = d.src_off;
    s.cand[0] = s.cand[1] = lz86::kNone;
    LzmaEncGpuStreamDesc& t = j.tmpl[i];
    memset(&t, 0, sizeof(t));
    t.src_len = d.src_len;
    if (d.dst_cap < LZMA86_HEADER_SIZE) {
      s.pre = SZ_ERROR_OUTPUT_EOF;
      continue;
    }
    lzenc::EncProps e;
    lzenc::props_init(&e);
    e.level = d.level;
    e.dictSize = d.dictSize;
    lzenc::Params q;
    const char* field = nullptr;
    const int32_t pr = lzenc::params_from_props_ex(&e, 0, allowed, &q, &field);
    if (pr == lzenc::kErrUnsupported) lzmaenc_set_unsupported_error(field);
    if (pr != lzenc::kOk) {
      s.pre = pr;
      continue;
    }
    if (d.src_len >= (uint64_t(1) << 31)) {
      set_error("Lzma86 encode: a source of 2^31 bytes or more is not supported");
      s.pre = SZ_ERROR_UNSUPPORTED;
      continue;
    }
    s.pre = SZ_OK;
    lzenc::write_props5(q, s.props5);
    t.dict_size = q.dict_size;
    t.lc = q.lc;
    t.lp = q.lp;
    t.pb = q.pb;
    t.fb = q.fb;
    t.mc = q.mc;
    t.write_end_mark = 0;
    t.mode = lzenc::mode_of(q);
    t.dst_cap = d.dst_cap - LZMA86_HEADER_SIZE;
    j.slice[i] = lzmaenc_slice_bytes(t);
    j.has_f[i] = d.filterMode != SZ_FILTER_NO;
    j.has_u[i] = d.filterMode == SZ_FILTER_NO || d.filterMode == SZ_FILTER_AUTO;
  }
}
uint64_t enc_work(const EncJob& j, size_t i) {
  return j.n_cand(i) ? lzmaenc_work(j.tmpl[i]) : 0;
}
uint64_t enc_slice(const EncJob& j, size_t i) { return j.n_cand(i) * j.slice[i]; }

// the candidates in the plan's order (a stream's two side by side), their slots,
// the filter area and the scratch layout
void enc_layout(const Lzma86GpuStreamDesc* descs, EncJob& j, uint64_t split) {
  const size_t n = j.n;
  j.cand_start.assign(n + 1, 0);
  j.filt_off.assign(n, 0);
  uint64_t slots = 0, filt = 0;
  size_t m = 0;
  for (size_t k = 0; k < n; ++k) {
    const size_t i = j.plan.order[k];
    lz86::Stream& s = j.streams[i];
    j.cand_start[k] = m;
    const uint64_t room = s.pre == SZ_OK ? s.dst_cap - LZMA86_HEADER_SIZE : 0;
    for (int c = 0; c < 2; ++c) {
      if (!(c ? j.has_f[i] : j.has_u[i])) continue;
      s.cand[c] = uint32_t(m++);
      s.slot_off[c] = slots;
      slots += up(room, 16);
    }
    if (j.has_f[i]) {
      j.filt_off[i] = filt;
      lz86::StageJob q;
      q.src_off = descs[i].src_off;
      q.dst_off = filt;
      q.len = s.src_len;
      j.stage.push_back(q);
      j.max_stage = std::max(j.max_stage, q.len);
      filt += up(s.src_len, 16);
    }
  }
  j.cand_start[n] = m;
  for (size_t i = 0; i < n; ++i) {  // caller order: the gather walks the list
    const lz86::Stream& s = j.streams[i];
    if (j.n_cand(i) && s.dst_cap - LZMA86_HEADER_SIZE > split) {
      j.large.push_back(uint32_t(i));
      j.max_large = std::max(j.max_large, s.dst_cap - LZMA86_HEADER_SIZE);
    }
  }
  j.filt_bytes = filt;
  j.slots_bytes = slots;
  Place p;
  const size_t nf = j.stage.size();
  j.o_streams = p.take(n * sizeof(lz86::Stream));
  j.o_cands = p.take(m * sizeof(LzmaEncGpuStreamDesc));
  j.o_cres = p.take(m * sizeof(LzmaEncGpuResult));
  j.o_stage = p.take(nf * sizeof(lz86::StageJob));
  j.o_r64 = p.take(3 * nf * sizeof(uint64_t));
  j.o_r32 = p.take(2 * nf * sizeof(uint32_t));
  j.o_large = p.take(j.large.size() * sizeof(uint32_t));
  j.o_filt = p.take(filt + 16);
  j.o_slots = p.take(slots + 16);
  j.o_ws = p.take(j.plan.ws_max);
  j.total = p.total;
}

uint32_t parts_of(uint64_t longest) {
  const uint64_t parts = (longest + kLzma86PartBytes - 1) / kLzma86PartBytes;
  return uint32_t(std::min<uint64_t>(std::max<uint64_t>(parts, 1), kLzma86PartsMax));
}

struct StageClock {
  Lzma86GpuStats* stats;
  hipStream_t stream;
  uint64_t t0;
  bool on() const { return stats && (stats->flags & LZMA86_GPU_TIMINGS); }
  // the stage's queued work has finished
  bool mark(unsigned stage) {
    if (!on()) return true;
    if (!hip_ok(hipStreamSynchronize(stream), "Lzma86 stage")) return false;
    const uint64_t t = now_ns();
    stats->stage_ns[stage] += t - t0;
    t0 = t;
    return true;
  }
};

// Everything of one batch on `stream`; the tables go up in one blocking copy.
SRes enc_queue(const EncJob& j, const Byte* d_src, Byte* d_dst, uint8_t* scratch,
               Lzma86GpuResult* d_results, hipStream_t stream, Lzma86GpuStats* stats,
               uint64_t split) {
  static const char what[] = "Lzma86 encode batch";
  const size_t n = j.n, m = j.candidates(), nf = j.stage.size();
  uint8_t* filt = scratch + j.o_filt;
  uint8_t* slots = scratch + j.o_slots;
  // the encoder takes one source base: the lower of the caller's source and the
  // filter area, the candidates' offsets counted from it
  const uintptr_t a_src = reinterpret_cast<uintptr_t>(d_src);
  const uintptr_t a_filt = reinterpret_cast<uintptr_t>(filt);
  const uintptr_t a_base = std::min(a_src, a_filt);
  const uint8_t* src_base = reinterpret_cast<const uint8_t*>(a_base);
  std::vector<uint8_t> img(size_t(j.o_filt), 0);
  if (n) memcpy(img.data() + j.o_streams, j.streams.data(), n * sizeof(lz86::Stream));
  LzmaEncGpuStreamDesc* cands = reinterpret_cast<LzmaEncGpuStreamDesc*>(img.data() + j.o_cands);
  for (size_t k = 0; k < n; ++k) {
    const size_t i = j.plan.order[k];
    const lz86::Stream& s = j.streams[i];
    uint64_t ws = j.plan.ws_off[k];
    for (int c = 0; c < 2; ++c) {
      if (s.cand[c] == lz86::kNone) continue;
      LzmaEncGpuStreamDesc d = j.tmpl[i];
      d.src_off = c ? uint64_t(a_filt - a_base) + j.filt_off[i]
                    : uint64_t(a_src - a_base) + j.src_off[i];
      d.dst_off = s.slot_off[c];
      d.ws_off = ws;
      ws += j.slice[i];
      cands[s.cand[c]] = d;
    }
  }
  if (nf) {
    memcpy(img.data() + j.o_stage, j.stage.data(), nf * sizeof(lz86::StageJob));
    uint64_t* r64 = reinterpret_cast<uint64_t*>(img.data() + j.o_r64);
    for (size_t f = 0; f < nf; ++f) {
      r64[f] = j.stage[f].dst_off;
      r64[nf + f] = j.stage[f].len;
    }
  }
  if (!j.large.empty())
    memcpy(img.data() + j.o_large, j.large.data(), j.large.size() * sizeof(uint32_t));
  if (!img.empty() &&
      !hip_ok(hipMemcpy(scratch, img.data(), img.size(), hipMemcpyHostToDevice), "upload tables"))
    return SZ_ERROR_FAIL;
  StageClock clock{stats, stream, now_ns()};

  if (nf) {
    if (lzma86gpu_launch_stage(reinterpret_cast<const lz86::StageJob*>(scratch + j.o_stage),
                               uint32_t(nf), parts_of(j.max_stage), d_src, filt, stream) != 0) {
      set_error("Lzma86 stage kernel launch failed");
      return SZ_ERROR_FAIL;
    }
    uint64_t* r64 = reinterpret_cast<uint64_t*>(scratch + j.o_r64);
    uint32_t* r32 = reinterpret_cast<uint32_t*>(scratch + j.o_r32);
    const SRes fr = BcjGpu_X86Batch(filt, r64, r64 + nf, r32, r32 + nf, r64 + 2 * nf, nf, 1, stream);
    if (fr != SZ_OK) return fr;
  }
  if (!clock.mark(LZMA86_GPU_STAGE_FILTER)) return SZ_ERROR_FAIL;

  const LzmaEncGpuStreamDesc* d_cands =
      reinterpret_cast<const LzmaEncGpuStreamDesc*>(scratch + j.o_cands);
  LzmaEncGpuResult* d_cres = reinterpret_cast<LzmaEncGpuResult*>(scratch + j.o_cres);
  uint64_t launches = 0;
  const SRes qr = queue_launches(what, j.plan, [&](uint32_t lo, uint32_t cnt) {
    const size_t c0 = j.cand_start[lo], c1 = j.cand_start[lo + cnt];
    if (c0 == c1) return 0;
    ++launches;
    return lzmaencgpu_launch(d_cands + c0, nullptr, uint32_t(c1 - c0), src_base, slots,
                             scratch + j.o_ws, d_cres + c0, LZMA_ENC_GPU_LANES_DEFAULT, stream,
                             lzmaenc_kernels(cands + c0, c1 - c0, lzmaenc_check));
  });
  if (qr != SZ_OK) return qr;
  if (!clock.mark(LZMA86_GPU_STAGE_ENCODE)) return SZ_ERROR_FAIL;

  if (lzma86gpu_launch_select(reinterpret_cast<const lz86::Stream*>(scratch + j.o_streams),
                              uint32_t(n), d_cres, slots, d_dst, d_results,
                              reinterpret_cast<const uint32_t*>(scratch + j.o_large),
                              uint32_t(j.large.size()), parts_of(j.max_large), split,
                              stream) != 0) {
    set_error("Lzma86 select kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  if (!clock.mark(LZMA86_GPU_STAGE_SELECT)) return SZ_ERROR_FAIL;
  if (stats) {
    stats->candidates = m;
    stats->filtered = nf;
    stats->encode_launches = launches;
  }
  (void)m;
  return SZ_OK;
}

// one_item: dst is not uploaded and only the stream's bytes come back (the
// drop-in's dest may be far larger than the stream)
SRes encode_batch_host(const Lzma86GpuStreamDesc* descs, size_t n, const Byte* src,
                       size_t src_size, Byte* dst, size_t dst_size, Lzma86GpuResult* results,
                       uint64_t workspace_limit, Lzma86GpuStats* stats, bool one_item) {
  static const char what[] = "Lzma86 encode batch";
  const uint64_t t_call = now_ns();
  if (stats) {
    const uint32_t flags = stats->flags;
    memset(stats, 0, sizeof(*stats));
    stats->flags = flags;
  }
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n == 0) return SZ_OK;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  EncJob j;
  enc_streams(descs, n, j);
  Batch b;
  SRes r = b.lay_out(
      what, descs, n, src_size, dst_size, workspace_limit,
      [](const Lzma86GpuStreamDesc& d) { return d.dst_cap; },
      [&](const Lzma86GpuStreamDesc& d) { return enc_work(j, size_t(&d - descs)); },
      [&](const Lzma86GpuStreamDesc& d) { return enc_slice(j, size_t(&d - descs)); });
  if (r != SZ_OK) return r;
  j.plan = b.plan;
  const uint64_t split = lzma86_split();
  enc_layout(descs, j, split);
  if ((r = alloc_all(what, b.src, src_size, b.dst, dst_size, b.ws, size_t(j.total), b.res, n)) !=
      SZ_OK)
    return r;
  if (!hip_ok(hipMemcpy(b.src.p, src, src_size, hipMemcpyHostToDevice), "upload src") ||
      (!one_item &&
       !hip_ok(hipMemcpy(b.dst.p, dst, dst_size, hipMemcpyHostToDevice), "upload dst")))
    return SZ_ERROR_FAIL;
  if ((r = enc_queue(j, b.src.p, b.dst.p, b.ws.p, b.res.p, nullptr, stats, split)) != SZ_OK ||
      (r = b.wait(what, results, n)) != SZ_OK)
    return r;
  const size_t off = one_item ? size_t(descs[0].dst_off) : 0;
  const size_t len =
      one_item ? size_t(std::min<uint64_t>(results[0].dest_len, descs[0].dst_cap)) : dst_size;
  if (!b.download_dst(dst, off, len)) return SZ_ERROR_FAIL;
  if (stats) stats->stage_ns[LZMA86_GPU_STAGE_TOTAL] = now_ns() - t_call;
  return SZ_OK;
}

// ---------------------------------------------------------------- decode

struct DecJob {
  size_t n = 0;
  std::vector<lz86::DecStream> streams;
  std::vector<LzmaGpuStreamDesc> lzma;
  std::vector<uint32_t> order;
  std::vector<uint64_t> x86_off;
  uint64_t ws_bytes = 0;
  uint64_t o_streams = 0, o_lzma = 0, o_order = 0, o_lres = 0, o_r64 = 0, o_r32 = 0, o_ws = 0,
           total = 0;
};

// Lzma86_Decode's checks of the header, then the payload as one LZMA stream
void dec_prepare(const Lzma86GpuStreamDesc* descs, size_t n, const Byte* headers, DecJob& j) {
  j.n = n;
  j.streams.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const Lzma86GpuStreamDesc& d = descs[i];
    const Byte* h = headers + LZMA86_HEADER_SIZE * i;
    lz86::DecStream& s = j.streams[i];
    s.slot = s.range = lz86::kNone;
    s.filter = 0;
    s.pre = SZ_OK;
    if (d.src_len < LZMA86_HEADER_SIZE) {
      s.pre = SZ_ERROR_INPUT_EOF;
      continue;
    }
    s.filter = h[0];
    if (h[0] > 1) {
      s.pre = SZ_ERROR_UNSUPPORTED;
      continue;
    }
    LzmaGpuStreamDesc q;
    memset(&q, 0, sizeof(q));
    q.src_off = d.src_off + LZMA86_HEADER_SIZE;
    q.src_len = d.src_len - LZMA86_HEADER_SIZE;
    q.dst_off = d.dst_off;
    q.dst_cap = d.dst_cap;
    memcpy(q.props, h + 1, LZMA_PROPS_SIZE);
    q.props_size = LZMA_PROPS_SIZE;
    q.finish_mode = LZMA_FINISH_ANY;
    q.kind = LZMA_GPU_KIND_LZMA;
    s.slot = uint32_t(j.lzma.size());
    j.lzma.push_back(q);
    if (h[0] == 1) {
      s.range = uint32_t(j.x86_off.size());
      j.x86_off.push_back(d.dst_off);
    }
  }
  const size_t m = j.lzma.size(), nr = j.x86_off.size();
  j.order.resize(m);
  j.ws_bytes = LzmaGpu_PlanBatch(j.lzma.data(), m, j.order.data());
  Place p;
  j.o_streams = p.take(n * sizeof(lz86::DecStream));
  j.o_lzma = p.take(m * sizeof(LzmaGpuStreamDesc));
  j.o_order = p.take(m * sizeof(uint32_t));
  j.o_lres = p.take(m * sizeof(LzmaGpuResult));
  j.o_r64 = p.take(3 * nr * sizeof(uint64_t));
  j.o_r32 = p.take(2 * nr * sizeof(uint32_t));
  j.o_ws = p.take(j.ws_bytes);
  j.total = p.total;
}

SRes dec_queue(const DecJob& j, const Byte* d_src, Byte* d_dst, uint8_t* scratch,
               Lzma86GpuResult* d_results, hipStream_t stream) {
  const size_t n = j.n, m = j.lzma.size(), nr = j.x86_off.size();
  std::vector<uint8_t> img(size_t(j.o_ws), 0);
  if (n) memcpy(img.data() + j.o_streams, j.streams.data(), n * sizeof(lz86::DecStream));
  if (m) {
    memcpy(img.data() + j.o_lzma, j.lzma.data(), m * sizeof(LzmaGpuStreamDesc));
    memcpy(img.data() + j.o_order, j.order.data(), m * sizeof(uint32_t));
  }
  if (nr) memcpy(img.data() + j.o_r64, j.x86_off.data(), nr * sizeof(uint64_t));
  if (!img.empty() &&
      !hip_ok(hipMemcpy(scratch, img.data(), img.size(), hipMemcpyHostToDevice), "upload tables"))
    return SZ_ERROR_FAIL;
  LzmaGpuResult* d_lres = reinterpret_cast<LzmaGpuResult*>(scratch + j.o_lres);
  uint64_t* r64 = reinterpret_cast<uint64_t*>(scratch + j.o_r64);
  uint32_t* r32 = reinterpret_cast<uint32_t*>(scratch + j.o_r32);
  if (m) {
    const SRes r = LzmaGpu_DecodeBatch(
        reinterpret_cast<const LzmaGpuStreamDesc*>(scratch + j.o_lzma),
        reinterpret_cast<const uint32_t*>(scratch + j.o_order), m, d_src, d_dst, scratch + j.o_ws,
        size_t(j.ws_bytes), d_lres, stream);
    if (r != SZ_OK) return r;
  }
  if (lzma86gpu_launch_finish(reinterpret_cast<const lz86::DecStream*>(scratch + j.o_streams),
                              uint32_t(n), d_lres, d_results, r64 + nr, stream) != 0) {
    set_error("Lzma86 finish kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  if (nr == 0) return SZ_OK;
  return BcjGpu_X86Batch(d_dst, r64, r64 + nr, r32, r32 + nr, r64 + 2 * nr, nr, 0, stream);
}

SRes decode_batch_host(const Lzma86GpuStreamDesc* descs, size_t n, const Byte* src, size_t src_size,
                       Byte* dst, size_t dst_size, Lzma86GpuResult* results, bool one_item) {
  static const char what[] = "Lzma86 decode batch";
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n == 0) return SZ_OK;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  std::vector<Byte> headers(n * LZMA86_HEADER_SIZE, 0);
  for (size_t i = 0; i < n; ++i) {
    const Lzma86GpuStreamDesc& d = descs[i];
    if (d.src_off > src_size || d.src_len > src_size - d.src_off || d.dst_off > dst_size ||
        d.dst_cap > dst_size - d.dst_off)
      return SZ_ERROR_PARAM;
    memcpy(headers.data() + LZMA86_HEADER_SIZE * i, src + d.src_off,
           size_t(std::min<uint64_t>(d.src_len, LZMA86_HEADER_SIZE)));
  }
  DecJob j;
  dec_prepare(descs, n, headers.data(), j);
  Batch b;
  SRes r = alloc_all(what, b.src, src_size, b.dst, dst_size, b.ws, size_t(j.total), b.res, n);
  if (r != SZ_OK) return r;
  if (!hip_ok(hipMemcpy(b.src.p, src, src_size, hipMemcpyHostToDevice), "upload src") ||
      (!one_item &&
       !hip_ok(hipMemcpy(b.dst.p, dst, dst_size, hipMemcpyHostToDevice), "upload dst")))
    return SZ_ERROR_FAIL;
  if ((r = dec_queue(j, b.src.p, b.dst.p, b.ws.p, b.res.p, nullptr)) != SZ_OK ||
      (r = b.wait(what, results, n)) != SZ_OK)
    return r;
  const size_t off = one_item ? size_t(descs[0].dst_off) : 0;
  const size_t len =
      one_item ? size_t(std::min<uint64_t>(results[0].dest_len, descs[0].dst_cap)) : dst_size;
  return b.download_dst(dst, off, len) ? SZ_OK : SZ_ERROR_FAIL;
}

}  // namespace

extern "C" SRes Lzma86Gpu_EncodeScratch(const Lzma86GpuStreamDesc* descs, size_t n,
                                        uint64_t* scratch_bytes) {
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  return guarded("Lzma86 encode plan: host allocation failed", [&]() -> SRes {
    EncJob j;
    enc_streams(descs, n, j);
    launch_plan(n, [&](uint32_t i) { return enc_work(j, i); },
                [&](uint32_t i) { return enc_slice(j, i); }, ~uint64_t(0), j.plan);
    enc_layout(descs, j, lzma86_split());
    *scratch_bytes = j.total;
    return SZ_OK;
  });
}

extern "C" SRes Lzma86Gpu_EncodeBatch(const Lzma86GpuStreamDesc* descs, size_t n,
                                      const Byte* d_src, Byte* d_dst, void* d_scratch,
                                      uint64_t scratch_bytes, Lzma86GpuResult* d_results,
                                      void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (n == 0) return SZ_OK;
  return guarded("Lzma86 encode batch: host allocation failed", [&]() -> SRes {
    EncJob j;
    enc_streams(descs, n, j);
    launch_plan(n, [&](uint32_t i) { return enc_work(j, i); },
                [&](uint32_t i) { return enc_slice(j, i); }, ~uint64_t(0), j.plan);
    const uint64_t split = lzma86_split();
    enc_layout(descs, j, split);
    if (scratch_bytes < j.total) return SZ_ERROR_PARAM;
    return enc_queue(j, d_src, d_dst, static_cast<uint8_t*>(d_scratch), d_results,
                     static_cast<hipStream_t>(stream), nullptr, split);
  });
}

extern "C" SRes Lzma86Gpu_EncodeBatchHost(const Lzma86GpuStreamDesc* descs, size_t n,
                                          const Byte* src, size_t src_size, Byte* dst,
                                          size_t dst_size, Lzma86GpuResult* results,
                                          uint64_t workspace_limit, Lzma86GpuStats* stats) {
  return guarded("Lzma86 encode batch: host allocation failed", [&]() {
    return encode_batch_host(descs, n, src, src_size, dst, dst_size, results, workspace_limit,
                             stats, false);
  });
}

extern "C" SRes Lzma86Gpu_DecodeScratch(const Lzma86GpuStreamDesc* descs, size_t n,
                                        const Byte* headers, uint64_t* scratch_bytes) {
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  return guarded("Lzma86 decode plan: host allocation failed", [&]() -> SRes {
    DecJob j;
    dec_prepare(descs, n, headers, j);
    *scratch_bytes = j.total;
    return SZ_OK;
  });
}

extern "C" SRes Lzma86Gpu_DecodeBatch(const Lzma86GpuStreamDesc* descs, size_t n,
                                      const Byte* headers, const Byte* d_src, Byte* d_dst,
                                      void* d_scratch, uint64_t scratch_bytes,
                                      Lzma86GpuResult* d_results, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (n == 0) return SZ_OK;
  return guarded("Lzma86 decode batch: host allocation failed", [&]() -> SRes {
    DecJob j;
    dec_prepare(descs, n, headers, j);
    if (scratch_bytes < j.total) return SZ_ERROR_PARAM;
    return dec_queue(j, d_src, d_dst, static_cast<uint8_t*>(d_scratch), d_results,
                     static_cast<hipStream_t>(stream));
  });
}

extern "C" SRes Lzma86Gpu_DecodeBatchHost(const Lzma86GpuStreamDesc* descs, size_t n,
                                          const Byte* src, size_t src_size, Byte* dst,
                                          size_t dst_size, Lzma86GpuResult* results) {
  return guarded("Lzma86 decode batch: host allocation failed", [&]() {
    return decode_batch_host(descs, n, src, src_size, dst, dst_size, results, false);
  });
}

extern "C" SRes Lzma86_Encode(Byte* dest, size_t* destLen, const Byte* src, size_t srcLen,
                              int level, UInt32 dictSize, int filterMode) {
  const size_t cap = *destLen;
  *destLen = 0;
  if (cap < LZMA86_HEADER_SIZE) return SZ_ERROR_OUTPUT_EOF;
  Lzma86GpuStreamDesc d;
  memset(&d, 0, sizeof(d));
  d.src_len = srcLen;
  d.dst_cap = cap;
  d.level = level;
  d.dictSize = dictSize;
  d.filterMode = filterMode;
  Lzma86GpuResult r;
  r.res = SZ_ERROR_FAIL;
  r.dest_len = 0;
  const SRes res = guarded("Lzma86 encode: host allocation failed", [&]() {
    return encode_batch_host(&d, 1, src, srcLen, dest, cap, &r, 0, nullptr, true);
  });
  if (res != SZ_OK) return res;
  *destLen = size_t(r.dest_len);
  return r.res;
}

extern "C" SRes Lzma86_GetUnpackSize(const Byte* src, SizeT srcLen, UInt64* unpackSize) {
  if (srcLen < LZMA86_HEADER_SIZE) return SZ_ERROR_INPUT_EOF;
  *unpackSize = 0;
  for (unsigned i = 0; i < sizeof(UInt64); i++)
    *unpackSize += UInt64(src[LZMA86_SIZE_OFFSET + i]) << (8 * i);
  return SZ_OK;
}

extern "C" SRes Lzma86_Decode(Byte* dest, SizeT* destLen, const Byte* src, SizeT* srcLen) {
  if (*srcLen < LZMA86_HEADER_SIZE) return SZ_ERROR_INPUT_EOF;
  if (src[0] > 1) {
    *destLen = 0;
    return SZ_ERROR_UNSUPPORTED;
  }
  Lzma86GpuStreamDesc d;
  memset(&d, 0, sizeof(d));
  d.src_len = *srcLen;
  d.dst_cap = *destLen;
  Lzma86GpuResult r;
  r.res = SZ_ERROR_FAIL;
  r.dest_len = r.src_len = 0;
  const SRes res = guarded("Lzma86 decode: host allocation failed", [&]() {
    return decode_batch_host(&d, 1, src, *srcLen, dest, *destLen, &r, true);
  });
  if (res != SZ_OK) return res;
  *destLen = SizeT(r.dest_len);
  *srcLen = SizeT(r.src_len);
  return r.res;
}
