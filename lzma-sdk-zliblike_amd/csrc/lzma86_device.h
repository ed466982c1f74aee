// lzma86_device.h -- the device side of the Lzma86 batch (Lzma86Enc.c,
// Lzma86Dec.c): the copy of the sources that get a filtered candidate, the
// choice between a stream's candidates with the 14 header bytes, the gather of
// the chosen candidate into the caller's slot, and the decoder's last step.
// Shared by lzma86_kernels.hip (thin wrappers: one call per thread) and by host
// code, which can run the same functions thread by thread.
//
//   stage    one workgroup per (job, part): a source range copied into the
//            filter area, where BcjGpu_X86Batch converts it in place
//   select   one wave per stream: both candidates' results read, the rule of
//            Lzma86_Encode applied, header and result written by lane 0, the
//            chosen candidate moved when it is at most `split` bytes
//   gather   one workgroup per (listed stream, part): the same choice again,
//            the chosen candidate moved when it is longer than `split`
//   finish   (decode) one thread per stream: the LZMA result turned into the
//            stream's result and into the range the x86 filter runs over
//
// The moves are sevenz_pack_device.h's: 16-byte stores aligned to the
// destination, each made from two aligned 16-byte loads, head and tail by
// bytes; here with a thread count and a share of the vectors given by the
// caller.  Nothing outside [dst_off, dst_off + dst_cap) is written.
#pragma once

#include <stdint.h>

#include "../../include/lzma_gpu.h"
#include "sevenz_pack_device.h"

namespace lz86 {

constexpr int32_t kOk = 0, kErrOutputEof = 7;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kHeader = 14;
constexpr uint32_t kThreads = 256;  // threads of a workgroup
constexpr uint32_t kWave = 64;

// One stream as the select and gather kernels see it (64 bytes).
struct Stream {
  uint64_t dst_off, dst_cap;  // the caller's slot in d_dst
  uint64_t src_len;
  uint64_t slot_off[2];       // candidate slots in the slot area: unfiltered, filtered
  uint32_t cand[2];           // their index in the candidates' results, kNone: none
  int32_t pre;                // kOk, or the host's verdict: nothing is written
  uint8_t props5[5];
  uint8_t pad[3];
};

// One range of the stage kernel (24 bytes).
struct StageJob {
  uint64_t src_off;  // from the source base
  uint64_t dst_off;  // from the filter area
  uint64_t len;
};

// One stream of the decode finish (16 bytes).
struct DecStream {
  uint32_t slot;    // index in the LZMA decode batch, kNone: pre is the result
  int32_t pre;
  uint32_t filter;  // the flag byte
  uint32_t range;   // index of its x86 range, kNone: none
};

struct Choice {
  int32_t res;
  uint32_t filter;  // the flag byte
  uint64_t len;     // payload bytes
};

// Lzma86_Encode's passes over the candidates that exist: a candidate counts
// when it fitted (SZ_OK); the filtered one wins only when it is strictly
// smaller than an unfiltered one that fitted; with none the verdict is the
// first other error, else SZ_ERROR_OUTPUT_EOF, flag 0, no payload.
SZPACK_FN Choice choose(const Stream& s, const LzmaEncGpuResult* cand) {
  Choice c;
  c.res = kErrOutputEof;
  c.filter = 0;
  c.len = 0;
  const bool has_u = s.cand[0] != kNone, has_f = s.cand[1] != kNone;
  LzmaEncGpuResult u, f;
  u.res = f.res = kErrOutputEof;
  u.dest_len = f.dest_len = 0;
  if (has_u) u = cand[s.cand[0]];
  if (has_f) f = cand[s.cand[1]];
  const uint64_t room = s.dst_cap - kHeader;
  const bool u_ok = has_u && u.res == kOk && u.dest_len <= room;
  const bool f_ok = has_f && f.res == kOk && f.dest_len <= room;
  if (f_ok && (!u_ok || f.dest_len < u.dest_len)) {
    c.res = kOk;
    c.filter = 1;
    c.len = f.dest_len;
  } else if (u_ok) {
    c.res = kOk;
    c.len = u.dest_len;
  } else if (has_f && f.res != kOk && f.res != kErrOutputEof) {
    c.res = f.res;
  } else if (has_u && u.res != kOk && u.res != kErrOutputEof) {
    c.res = u.res;
  }
  return c;
}

// where the chosen candidate lies (no indexed access: the stream stays in registers)
SZPACK_FN uint64_t slot_of(const Stream& s, const Choice& c) {
  return c.filter ? s.slot_off[1] : s.slot_off[0];
}

// lane 0 of the wave that has the stream: the header and the result
SZPACK_FN void write_header(const Stream& s, const Choice& c, uint8_t* d_dst,
                            Lzma86GpuResult* out) {
  out->src_len = 0;
  if (s.pre != kOk) {
    out->res = s.pre;
    out->filter = 0;
    out->dest_len = 0;
    return;
  }
  uint8_t* h = d_dst + s.dst_off;
  h[0] = uint8_t(c.filter);
  for (uint32_t i = 0; i < 5; ++i) h[1 + i] = s.props5[i];
  for (uint32_t i = 0; i < 8; ++i) h[6 + i] = uint8_t(s.src_len >> (8 * i));
  out->res = c.res;
  out->filter = c.filter;
  out->dest_len = kHeader + c.len;
  out->src_len = s.src_len;
}

// Thread t of nt moves share `part` of `parts` of len bytes from s to d (any
// alignment): part 0 has the head and the tail bytes, the 16-byte vectors are
// split evenly.  Both loads of a vector lie in aligned 16-byte granules that
// hold bytes of [s, s + len).
SZPACK_FN void move_part(const uint8_t* s, uint8_t* d, uint64_t len, uint32_t t, uint32_t nt,
                         uint64_t part, uint64_t parts) {
  using namespace szpack;
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
  if (head > len) head = len;
  const uint64_t vecs = (len - head) >> 4;
  const uint64_t tail_at = head + (vecs << 4);
  if (part == 0) {
    for (uint64_t i = t; i < head; i += nt) d[i] = s[i];
    for (uint64_t i = tail_at + t; i < len; i += nt) d[i] = s[i];
  }
  const uint64_t per = (vecs + parts - 1) / parts;
  const uint64_t lo = part * per < vecs ? part * per : vecs;
  const uint64_t hi = lo + per < vecs ? lo + per : vecs;
  if (lo >= hi) return;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s + head);
  const uint32_t sh = uint32_t(sa & 15);
  const uint8_t* sv = s + head - sh;
  uint8_t* dv = d + head;
  if (sh == 0) {
    for (uint64_t i = lo + t; i < hi; i += nt) store16(dv + (i << 4), load16(sv + (i << 4)));
    return;
  }
  const uint32_t word = sh >> 2, bits = (sh & 3) * 8;
  for (uint64_t i = lo + t; i < hi; i += nt) {
    const V16 a = load16(sv + (i << 4)), c = load16(sv + (i << 4) + 16);
    V16 v;
    switch (word) {  // uniform over the callers of one move
      case 0:
        v = V16{funnel(a.x, a.y, bits), funnel(a.y, a.z, bits), funnel(a.z, a.w, bits),
                funnel(a.w, c.x, bits)};
        break;
      case 1:
        v = V16{funnel(a.y, a.z, bits), funnel(a.z, a.w, bits), funnel(a.w, c.x, bits),
                funnel(c.x, c.y, bits)};
        break;
      case 2:
        v = V16{funnel(a.z, a.w, bits), funnel(a.w, c.x, bits), funnel(c.x, c.y, bits),
                funnel(c.y, c.z, bits)};
        break;
      default:
        v = V16{funnel(a.w, c.x, bits), funnel(c.x, c.y, bits), funnel(c.y, c.z, bits),
                funnel(c.z, c.w, bits)};
        break;
    }
    store16(dv + (i << 4), v);
  }
}

// select, lane t of the wave that has stream i
SZPACK_FN void select_thread(const Stream* streams, uint64_t i, const LzmaEncGpuResult* cand,
                             const uint8_t* d_slots, uint8_t* d_dst, Lzma86GpuResult* results,
                             uint64_t split, uint32_t t) {
  const Stream s = streams[i];
  Choice c;
  c.res = s.pre;
  c.filter = 0;
  c.len = 0;
  if (s.pre == kOk) c = choose(s, cand);
  if (t == 0) write_header(s, c, d_dst, &results[i]);
  if (s.pre != kOk || c.res != kOk || c.len == 0 || c.len > split) return;
  move_part(d_slots + slot_of(s, c), d_dst + s.dst_off + kHeader, c.len, t, kWave, 0, 1);
}

// gather, thread t of the workgroup that has share `part` of listed stream i
SZPACK_FN void gather_thread(const Stream* streams, uint64_t i, const LzmaEncGpuResult* cand,
                             const uint8_t* d_slots, uint8_t* d_dst, uint64_t split, uint32_t t,
                             uint64_t part, uint64_t parts) {
  const Stream s = streams[i];
  if (s.pre != kOk) return;
  const Choice c = choose(s, cand);
  if (c.res != kOk || c.len <= split) return;
  move_part(d_slots + slot_of(s, c), d_dst + s.dst_off + kHeader, c.len, t, kThreads,
            part, parts);
}

// stage, thread t of the workgroup that has share `part` of job j
SZPACK_FN void stage_thread(const StageJob* jobs, uint64_t j, const uint8_t* src_base,
                            uint8_t* filt_base, uint32_t t, uint64_t part, uint64_t parts) {
  const StageJob q = jobs[j];
  move_part(src_base + q.src_off, filt_base + q.dst_off, q.len, t, kThreads, part, parts);
}

// finish (decode), the thread that has stream i: Lzma86_Decode's outcome from
// LzmaDecode's, and the length of the range x86_Convert runs over
SZPACK_FN void finish_thread(const DecStream* streams, uint64_t i, const LzmaGpuResult* lzma,
                             Lzma86GpuResult* results, uint64_t* x86_len) {
  const DecStream s = streams[i];
  Lzma86GpuResult r;
  r.res = s.pre;
  r.filter = s.filter;
  r.dest_len = 0;
  r.src_len = 0;
  if (s.slot != kNone) {
    const LzmaGpuResult q = lzma[s.slot];
    r.res = q.res;
    r.dest_len = q.dest_len;
    r.src_len = q.src_len + kHeader;
  }
  if (s.range != kNone) x86_len[s.range] = r.res == kOk ? r.dest_len : 0;
  results[i] = r;
}

}  // namespace lz86
