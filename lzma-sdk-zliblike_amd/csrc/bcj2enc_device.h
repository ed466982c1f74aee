// bcj2enc_device.h -- the BCJ2 encoder: x86 code split into the four streams
// that bcj2_device.h (Bcj2.c:28-128) merges again.  The rule of tests/bcj2enc.py:
// a branch (E8, E9, 0F 8x) with its four operand bytes inside the stream is
// converted when its absolute target lies inside the stream.
//
//   isj(i)   (data[i] & 0xFE) == 0xE8, or data[i-1] == 0x0F and 8x
//   conv(i)  isj(i), i + 5 <= n, (i + 5 + rel) mod 2^32 < n
//   live     position i is live unless it is an operand byte of an earlier
//            live conv: s' = s > 0 ? s - 1 : (conv(i) ? 4 : 0), live iff s == 0
// isj and conv are functions of the source alone (the decoder's prevByte is
// always the preceding source byte), so only the five-state `s` is carried.
//
// A thread owns a run of kRun = 16 bytes, a wave a segment of 64 runs (1 KiB);
// segments, not streams, are handed to waves, so small streams share workgroups
// and a large stream spreads over the chip.  The scan element of a range of
// bytes is, PER ENTRY STATE s, one packed word
//     exit state (3 bits) | calls (9) | jumps (9) | bits (11)
// (live bytes follow: len - s - 4 (calls + jumps) + exit).  Kept per entry state
// because one backward pass over a run gives all five at once -- R[j] = the
// element of the run's suffix entered live at j is R[j + 5] + counts for a
// conv, R[j + 1] (+ a bit) otherwise, and entry state s is R[s] -- so the source
// is read twice (classify, scatter) where a map-first scan needs a third sweep
// for the counts.  Composition (f then g)[s] = (f[s] & ~7) + g[f[s] & 7] is
// associative; the fields cannot carry within a segment (<= 204 targets, <=
// 1,024 bits).  Across segments the maps alone are composed and the counts
// picked by entry state are added as 32-bit numbers (n < 2^31).
//
// Phases, each a function of (thread, phase) so that a host build
// (tests/emu_bcj2enc/) runs the same code thread by thread; every level across
// workgroups is its own launch and nothing waits on another workgroup:
//   plan      one workgroup: per stream its first segment and the start of its
//             scratch slice (exclusive scans over the streams), the totals
//   classify  per segment: run elements, a Hillis-Steele scan in LDS (two
//             buffers, a barrier per step), the segment's element
//   streams   one wave per stream, 64 segments per step: the maps composed,
//             the counts added; per segment its entry state and the targets
//             and bits before it; the stream's lengths
//   scatter   per segment: elements and scan again, then each thread walks its
//             run forward from its entry state: live bytes to main, targets
//             big-endian to call / jump, one 16-bit record (cell | bit << 15)
//             per decision to the stream's bit list in scratch
//   code      one lane per stream: the LZMA range encoder over the bit list,
//             258 lane-private cells; the result
// A write happens only below its stream's capacity (a target only whole); the
// result holds the four true lengths and SZ_ERROR_OUTPUT_EOF if one is above
// its capacity.  src_len >= 2^31: SZ_ERROR_UNSUPPORTED, nothing read or written.
//
// Scratch: Header | Info[n] | per stream: Elem[segs] | SegBase[segs] | uint16
// records[src_len], each part rounded up to 16 bytes.
#pragma once

#include <stdint.h>

#include "../../include/lzma_gpu.h"
#include "bcj2_device.h"

// BCJ2ENC_HD: sizes, on the host too; BCJ2ENC_FN: the phases (bcj2_device.h's
// helpers are device functions unless LZGPU_HOST_EMU makes them plain ones)
#if defined(__HIPCC__) && !defined(LZGPU_HOST_EMU)
#define BCJ2ENC_HD __host__ __device__ inline
#define BCJ2ENC_FN __device__ inline
#else
#define BCJ2ENC_HD inline
#define BCJ2ENC_FN inline
#endif

namespace bcj2enc {

constexpr uint32_t kRun = 16;                 // bytes of a thread's run
constexpr uint32_t kWave = 64;                // runs of a segment
constexpr uint32_t kSeg = kRun * kWave;       // bytes of a segment
constexpr uint32_t kWaves = 4;                // segments of a workgroup's step
constexpr uint32_t kThreads = kWave * kWaves;
constexpr uint32_t kScanSteps = 6;            // log2(kWave)
constexpr int32_t kOk = 0, kErrUnsupported = 4, kErrOutputEof = 7;
constexpr uint64_t kMaxLen = uint64_t(1) << 31;
constexpr uint32_t kCall = 1u << 3, kJump = 1u << 12, kBit = 1u << 21;
enum { kMain = 0, kCallS = 1, kJumpS = 2, kRc = 3 };

struct Elem {
  uint32_t v[5];
};
struct SegBase {
  uint32_t entry, calls, jumps, bits;  // the state entering the segment; counts before it
};
struct Header {
  uint64_t segs;  // of the whole batch
  uint64_t pad[7];
};
struct Info {  // 64 bytes per stream
  uint64_t seg_first;  // the stream's first segment in the batch
  uint64_t var_off;    // its slice in scratch
  uint32_t calls, jumps, bits, pad0;
  uint64_t pad[4];
};

struct Args {
  const Bcj2GpuEncDesc* descs;
  uint64_t n;
  const uint8_t* src;
  uint8_t* dst;
  uint8_t* scratch;
  Bcj2GpuEncResult* results;
};

BCJ2ENC_HD uint64_t up16(uint64_t v) { return (v + 15) & ~uint64_t(15); }
BCJ2ENC_HD uint64_t segs_of(uint64_t len) { return len >= kMaxLen ? 0 : (len + kSeg - 1) / kSeg; }
BCJ2ENC_HD uint64_t elems_bytes(uint64_t segs) { return up16(segs * sizeof(Elem)); }
BCJ2ENC_HD uint64_t var_bytes(uint64_t len) {
  if (len >= kMaxLen) return 0;
  const uint64_t s = segs_of(len);
  return elems_bytes(s) + s * sizeof(SegBase) + up16(len * 2);
}
BCJ2ENC_HD uint64_t slice_bytes(uint64_t len) { return sizeof(Info) + var_bytes(len); }
BCJ2ENC_HD uint64_t fixed_bytes() { return sizeof(Header); }

BCJ2ENC_FN Header* header_of(const Args& a) { return reinterpret_cast<Header*>(a.scratch); }
BCJ2ENC_FN Info* info_of(const Args& a) {
  return reinterpret_cast<Info*>(a.scratch + sizeof(Header));
}
BCJ2ENC_FN uint8_t* var_of(const Args& a, const Info& f) {
  return a.scratch + sizeof(Header) + a.n * sizeof(Info) + f.var_off;
}
BCJ2ENC_FN Elem* elems_of(const Args& a, const Info& f) {
  return reinterpret_cast<Elem*>(var_of(a, f));
}
BCJ2ENC_FN SegBase* bases_of(const Args& a, const Info& f, uint64_t segs) {
  return reinterpret_cast<SegBase*>(var_of(a, f) + elems_bytes(segs));
}
BCJ2ENC_FN uint16_t* recs_of(const Args& a, const Info& f, uint64_t segs) {
  return reinterpret_cast<uint16_t*>(var_of(a, f) + elems_bytes(segs) + segs * sizeof(SegBase));
}

// ---------------------------------------------------------------- plan

BCJ2ENC_FN void plan_run(const Args& a, uint32_t t, uint64_t* lo, uint64_t* hi) {
  const uint64_t per = (a.n + kThreads - 1) / kThreads;
  *lo = uint64_t(t) * per < a.n ? uint64_t(t) * per : a.n;
  *hi = *lo + per < a.n ? *lo + per : a.n;
}
// every thread: the segments and slice bytes of its run of streams
BCJ2ENC_FN void plan_part(const Args& a, uint32_t t, uint64_t* segs, uint64_t* bytes) {
  uint64_t lo, hi, s = 0, b = 0;
  plan_run(a, t, &lo, &hi);
  for (uint64_t k = lo; k < hi; ++k) {
    s += segs_of(a.descs[k].src_len);
    b += var_bytes(a.descs[k].src_len);
  }
  *segs = s;
  *bytes = b;
}
// thread 0 after the barrier: both arrays become exclusive; the batch's segments
BCJ2ENC_FN void plan_total(const Args& a, uint64_t* segs, uint64_t* bytes) {
  uint64_t s = 0, b = 0;
  for (uint32_t j = 0; j < kThreads; ++j) {
    const uint64_t vs = segs[j], vb = bytes[j];
    segs[j] = s;
    bytes[j] = b;
    s += vs;
    b += vb;
  }
  header_of(a)->segs = s;
}
// every thread after the second barrier
BCJ2ENC_FN void plan_write(const Args& a, uint32_t t, uint64_t segs, uint64_t bytes) {
  uint64_t lo, hi;
  plan_run(a, t, &lo, &hi);
  for (uint64_t k = lo; k < hi; ++k) {
    Info& f = info_of(a)[k];
    f.seg_first = segs;
    f.var_off = bytes;
    f.calls = f.jumps = f.bits = f.pad0 = 0;
    segs += segs_of(a.descs[k].src_len);
    bytes += var_bytes(a.descs[k].src_len);
  }
}

// the stream that holds segment `seg` (< the batch's segments): the last one
// whose first segment is <= seg (streams without segments share the first
// segment of the next stream that has some, and come before it)
BCJ2ENC_FN uint64_t stream_of(const Args& a, uint64_t seg) {
  const Info* f = info_of(a);
  uint64_t lo = 0, hi = a.n;  // f[lo].seg_first <= seg < f[hi].seg_first (hi == n: the end)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (f[mid].seg_first <= seg)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------- a run

// The run's 16 bytes, the 8 behind them and the byte before; bytes past the
// stream's end read as 0 (no branch opcode) and are never loaded.
struct Win {
  uint64_t w[3];
  uint32_t prev, len;
};

template <class B>
BCJ2ENC_FN Win load_win(const B* s, uint64_t n, uint64_t at) {
  Win x;
  x.w[0] = x.w[1] = x.w[2] = 0;
  x.prev = 0;
  x.len = 0;
  if (at >= n) return x;
  x.len = n - at < kRun ? uint32_t(n - at) : kRun;
  if (at) x.prev = uint32_t(s[at - 1]);
  if (n - at >= 24) {
    x.w[0] = lzgpu::bcj2_ld64(s + at);
    x.w[1] = lzgpu::bcj2_ld64(s + at + 8);
    x.w[2] = lzgpu::bcj2_ld64(s + at + 16);
  } else {
    for (uint32_t k = 0; k < 24; ++k)
      if (at + k < n) x.w[k >> 3] |= uint64_t(s[at + k]) << (8 * (k & 7));
  }
  return x;
}

BCJ2ENC_FN uint32_t win_byte(const Win& x, int j) {
  return uint32_t(x.w[j >> 3] >> (8 * (j & 7))) & 0xFFu;
}
// the little-endian dword at byte p <= 16 of the window
BCJ2ENC_FN uint32_t win_dword(const Win& x, int p) {
  const int k = p >> 3, sh = 8 * (p & 7);
  if (sh <= 32) return uint32_t(x.w[k] >> sh);
  return uint32_t((x.w[k] >> sh) | (x.w[k + 1] << (64 - sh)));
}
// 0x80 in byte j: position j of the run is a branch opcode
BCJ2ENC_FN void win_masks(const Win& x, uint64_t* m0, uint64_t* m1) {
  *m0 = lzgpu::bcj2_branch_mask(x.w[0], x.prev);
  *m1 = lzgpu::bcj2_branch_mask(x.w[1], uint32_t(x.w[0] >> 56));
}
BCJ2ENC_FN bool mask_at(uint64_t m0, uint64_t m1, int j) {
  return (((j < 8 ? m0 : m1) >> (8 * (j & 7) + 7)) & 1u) != 0;
}
// conv for the branch opcode at run position j (stream position at + j)
BCJ2ENC_FN bool conv_at(const Win& x, uint64_t n, uint64_t at, int j) {
  const uint64_t end = at + uint64_t(j) + 5;
  return end <= n && uint64_t(uint32_t(win_dword(x, j + 1) + uint32_t(end))) < n;
}

// the run's element: the backward pass of the header comment
BCJ2ENC_FN Elem run_elem(const Win& x, uint64_t n, uint64_t at) {
  Elem e;
  uint64_t m0, m1;
  win_masks(x, &m0, &m1);
  if ((m0 | m1) == 0 && x.len == kRun) {
    for (int s = 0; s < 5; ++s) e.v[s] = 0;
    return e;
  }
  uint32_t r[kRun + 5];
  const int len = int(x.len);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = kRun + 4; j >= int(kRun); --j) r[j] = uint32_t(j - len) & 7u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = kRun - 1; j >= 0; --j) {
    uint32_t v;
    if (j >= len) {
      v = uint32_t(j - len) & 7u;
    } else if (!mask_at(m0, m1, j)) {
      v = r[j + 1];
    } else if (conv_at(x, n, at, j)) {
      v = r[j + 5] + (win_byte(x, j) == 0xE8u ? kCall : kJump) + kBit;
    } else {
      v = r[j + 1] + (at + uint64_t(j) + 1 < n ? kBit : 0u);
    }
    r[j] = v;
  }
  for (int s = 0; s < 5; ++s) e.v[s] = r[s];
  return e;
}

BCJ2ENC_FN uint32_t pick(const Elem& g, uint32_t s) {
  return s == 0 ? g.v[0] : s == 1 ? g.v[1] : s == 2 ? g.v[2] : s == 3 ? g.v[3] : g.v[4];
}
// f, then g
BCJ2ENC_FN Elem compose(const Elem& f, const Elem& g) {
  Elem h;
  for (int s = 0; s < 5; ++s) h.v[s] = (f.v[s] & ~7u) + pick(g, f.v[s] & 7u);
  return h;
}
// step k of the inclusive scan over the kWave elements of `in`, lane `lane`
BCJ2ENC_FN void scan_step(const Elem* in, Elem* out, uint32_t lane, uint32_t k) {
  const uint32_t d = 1u << k;
  out[lane] = lane >= d ? compose(in[lane - d], in[lane]) : in[lane];
}
// where the scanned elements are after kScanSteps steps from buffer 0
constexpr uint32_t kScanOut = kScanSteps & 1;

// ---------------------------------------------------------------- classify, scatter

struct SegRef {
  uint64_t stream, seg;  // the stream and the segment within it
  uint64_t len;          // the stream's bytes (0: no such segment)
};
BCJ2ENC_FN SegRef seg_ref(const Args& a, uint64_t gseg) {
  SegRef r;
  r.stream = r.seg = r.len = 0;
  if (gseg >= header_of(a)->segs) return r;
  r.stream = stream_of(a, gseg);
  r.seg = gseg - info_of(a)[r.stream].seg_first;
  r.len = a.descs[r.stream].src_len;
  return r;
}

// classify and scatter, every thread: the element of its run (an idle thread's
// is the identity)
template <class B>
BCJ2ENC_FN Elem seg_elem(const Args& a, const SegRef& r, uint32_t lane, const B* src) {
  const uint64_t at = r.seg * kSeg + uint64_t(lane) * kRun;
  if (r.len == 0) {
    Elem e;
    for (int s = 0; s < 5; ++s) e.v[s] = uint32_t(s);
    return e;
  }
  const Win x = load_win(src + a.descs[r.stream].src_off, r.len, at);
  return run_elem(x, r.len, at);
}
// classify, the segment's last lane after the scan
BCJ2ENC_FN void classify_put(const Args& a, const SegRef& r, const Elem& total) {
  if (r.len == 0) return;
  elems_of(a, info_of(a)[r.stream])[r.seg] = total;
}

template <class B>
BCJ2ENC_FN void put_be32(B* p, uint32_t v) {
  p[0] = uint8_t(v >> 24);
  p[1] = uint8_t(v >> 16);
  p[2] = uint8_t(v >> 8);
  p[3] = uint8_t(v);
}

// scatter, every thread after the scan: `scanned` = the segment's inclusive scan
template <class B>
BCJ2ENC_FN void scatter_thread(const Args& a, const SegRef& r, uint32_t lane, const Elem* scanned,
                               const B* src, B* dst) {
  if (r.len == 0) return;
  const uint64_t n = r.len;
  const uint64_t at = r.seg * kSeg + uint64_t(lane) * kRun;
  if (at >= n) return;
  const Bcj2GpuEncDesc d = a.descs[r.stream];
  const Info& f = info_of(a)[r.stream];
  const uint64_t segs = segs_of(n);
  const SegBase sb = bases_of(a, f, segs)[r.seg];
  const uint32_t before = lane == 0 ? sb.entry : pick(scanned[lane - 1], sb.entry);
  uint32_t dead = before & 7u;
  uint64_t c = uint64_t(sb.calls) + ((before >> 3) & 0x1FFu);
  uint64_t jm = uint64_t(sb.jumps) + ((before >> 12) & 0x1FFu);
  uint64_t b = uint64_t(sb.bits) + (before >> 21);
  uint64_t m = at - (4 * (c + jm) - dead);  // live bytes before the run
  const Win x = load_win(src + d.src_off, n, at);
  uint64_t m0, m1;
  win_masks(x, &m0, &m1);
  B* mainp = dst + d.out[kMain].off;
  const uint64_t main_cap = d.out[kMain].cap;
  if ((m0 | m1) == 0 && x.len == kRun && dead == 0 && m + kRun <= main_cap) {
    lzgpu::bcj2_st64(mainp + m, x.w[0]);
    lzgpu::bcj2_st64(mainp + m + 8, x.w[1]);
    return;
  }
  uint16_t* recs = recs_of(a, f, segs);
  const int len = int(x.len);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < int(kRun); ++j) {
    const bool live = j < len && dead == 0;
    if (j < len && dead != 0) --dead;
    if (live) {
      const uint32_t byte = win_byte(x, j);
      if (m < main_cap) mainp[m] = uint8_t(byte);
      ++m;
      if (mask_at(m0, m1, j) && at + uint64_t(j) + 1 < n) {
        const bool cv = conv_at(x, n, at, j);
        const uint32_t prev = j == 0 ? x.prev : win_byte(x, j > 0 ? j - 1 : 0);
        const uint32_t cell = byte == 0xE8u ? prev : (byte == 0xE9u ? 256u : 257u);
        recs[b++] = uint16_t(cell | (cv ? 0x8000u : 0u));
        if (cv) {
          const uint32_t target = win_dword(x, j + 1) + uint32_t(at + uint64_t(j) + 5);
          if (byte == 0xE8u) {
            if (4 * c + 4 <= d.out[kCallS].cap)
              put_be32(dst + d.out[kCallS].off + 4 * c, target);
            ++c;
          } else {
            if (4 * jm + 4 <= d.out[kJumpS].cap)
              put_be32(dst + d.out[kJumpS].off + 4 * jm, target);
            ++jm;
          }
          dead = 4;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- streams

// One step of the stream scan covers kWave segments from `first`.  Lane:
// the map of its segment (the counts dropped), scanned like the runs'.
BCJ2ENC_FN Elem streams_map(const Args& a, uint64_t stream, uint64_t first, uint32_t lane) {
  const uint64_t segs = segs_of(a.descs[stream].src_len);
  Elem e;
  if (first + lane < segs) {
    e = elems_of(a, info_of(a)[stream])[first + lane];
    for (int s = 0; s < 5; ++s) e.v[s] &= 7u;
  } else {
    for (int s = 0; s < 5; ++s) e.v[s] = uint32_t(s);
  }
  return e;
}
// after the map scan: the lane's entry state under the step's entry state
// `carry`, and its segment's counts from there as an additive element
// (v[0..2] = calls, jumps, bits; v[3] = the entry state, not scanned)
BCJ2ENC_FN Elem streams_counts(const Args& a, uint64_t stream, uint64_t first, uint32_t lane,
                               const Elem* maps, uint32_t carry) {
  const uint64_t segs = segs_of(a.descs[stream].src_len);
  const uint32_t entry = lane == 0 ? carry : (pick(maps[lane - 1], carry) & 7u);
  Elem e;
  for (int s = 0; s < 5; ++s) e.v[s] = 0;
  e.v[3] = entry;
  if (first + lane < segs) {
    const uint32_t v = pick(elems_of(a, info_of(a)[stream])[first + lane], entry);
    e.v[0] = (v >> 3) & 0x1FFu;
    e.v[1] = (v >> 12) & 0x1FFu;
    e.v[2] = v >> 21;
  }
  return e;
}
BCJ2ENC_FN void add_step(const Elem* in, Elem* out, uint32_t lane, uint32_t k) {
  const uint32_t d = 1u << k;
  Elem e = in[lane];
  if (lane >= d)
    for (int s = 0; s < 3; ++s) e.v[s] += in[lane - d].v[s];
  out[lane] = e;
}
// after the additive scan (`own` = the lane's streams_counts element, `sums`
// inclusive): the segment's base under the counts `tot` before the step
BCJ2ENC_FN void streams_put(const Args& a, uint64_t stream, uint64_t first, uint32_t lane,
                              const Elem& own, const Elem* sums, const uint32_t* tot) {
  const uint64_t segs = segs_of(a.descs[stream].src_len);
  if (first + lane >= segs) return;
  SegBase sb;
  sb.entry = own.v[3];
  sb.calls = tot[0] + sums[lane].v[0] - own.v[0];
  sb.jumps = tot[1] + sums[lane].v[1] - own.v[1];
  sb.bits = tot[2] + sums[lane].v[2] - own.v[2];
  bases_of(a, info_of(a)[stream], segs)[first + lane] = sb;
}
// every lane after a step's two scans: the entry state and counts of the next
BCJ2ENC_FN void streams_next(const Elem* maps, const Elem* sums, uint32_t* carry, uint32_t* tot) {
  *carry = pick(maps[kWave - 1], *carry) & 7u;
  for (int s = 0; s < 3; ++s) tot[s] += sums[kWave - 1].v[s];
}
// lane 0 after the last step
BCJ2ENC_FN void streams_total(const Args& a, uint64_t stream, const uint32_t* tot) {
  Info& f = info_of(a)[stream];
  f.calls = tot[0];
  f.jumps = tot[1];
  f.bits = tot[2];
}

// ---------------------------------------------------------------- code

struct RangeEnc {
  uint64_t low, cache_size, pos;
  uint32_t range, cache;
};
template <class B>
BCJ2ENC_FN void rc_shift_low(RangeEnc& e, B* out, uint64_t cap) {
  if (uint32_t(e.low) < 0xFF000000u || uint32_t(e.low >> 32) != 0) {
    const uint32_t carry = uint32_t(e.low >> 32);
    uint32_t temp = e.cache;
    do {
      if (e.pos < cap) out[e.pos] = uint8_t(temp + carry);
      ++e.pos;
      temp = 0xFF;
    } while (--e.cache_size != 0);
    e.cache = uint32_t(e.low >> 24) & 0xFFu;
  }
  ++e.cache_size;
  e.low = uint64_t(uint32_t(e.low) & 0x00FFFFFFu) << 8;
}

// one lane: stream `stream`'s bit list through the range encoder, its result.
// prob: 258 lane-private cells.
template <class B, class P>
BCJ2ENC_FN void code_stream(const Args& a, uint64_t stream, B* dst, P prob) {
  const Bcj2GpuEncDesc d = a.descs[stream];
  Bcj2GpuEncResult res;
  res._pad = 0;
  for (int k = 0; k < 4; ++k) res.len[k] = 0;
  if (d.src_len >= kMaxLen) {
    res.res = kErrUnsupported;
    a.results[stream] = res;
    return;
  }
  const Info f = info_of(a)[stream];
  const uint16_t* recs = recs_of(a, f, segs_of(d.src_len));
  for (int i = 0; i < 258; ++i) prob[i] = uint16_t(1024);
  RangeEnc e;
  e.low = 0;
  e.range = 0xFFFFFFFFu;
  e.cache = 0;
  e.cache_size = 1;
  e.pos = 0;
  B* out = dst + d.out[kRc].off;
  const uint64_t cap = d.out[kRc].cap;
  for (uint32_t k = 0; k < f.bits; ++k) {
    const uint32_t rec = recs[k];
    const uint32_t cell = rec & 0x1FFu;
    const uint32_t p = prob[cell];
    const uint32_t bound = (e.range >> 11) * p;
    if (rec & 0x8000u) {
      e.low += bound;
      e.range -= bound;
      prob[cell] = uint16_t(p - (p >> 5));
    } else {
      e.range = bound;
      prob[cell] = uint16_t(p + ((2048u - p) >> 5));
    }
    while (e.range < (1u << 24)) {
      e.range <<= 8;
      rc_shift_low(e, out, cap);
    }
  }
  for (int i = 0; i < 5; ++i) rc_shift_low(e, out, cap);
  res.len[kMain] = d.src_len - 4 * (uint64_t(f.calls) + f.jumps);
  res.len[kCallS] = 4 * uint64_t(f.calls);
  res.len[kJumpS] = 4 * uint64_t(f.jumps);
  res.len[kRc] = e.pos;
  res.res = kOk;
  for (int k = 0; k < 4; ++k)
    if (res.len[k] > d.out[k].cap) res.res = kErrOutputEof;
  a.results[stream] = res;
}

}  // namespace bcj2enc
