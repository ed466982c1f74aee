// crc_device.h -- CRC-32 and CRC-64 of byte ranges on the GPU, one set of
// functions over the register type R.
//
// R = uint32_t: the reference's check after decode, CrcCalc (7zCrc.c:49-52:
// CrcUpdate from CRC_INIT_VAL 0xFFFFFFFF, result ^ 0xFFFFFFFF; reflected
// polynomial kCrcPoly 0xEDB88320, 7zCrc.c:7; byte step CRC_UPDATE_BYTE,
// 7zCrc.h:18; slice tables T[k][v] = T[0][T[k-1][v] & 0xFF] ^ (T[k-1][v] >> 8),
// 7zCrc.c:70-74).  Callers: 7zIn.c:1186, 1380, 1397 (folder and file CRCs).
// R = uint64_t: the xz block check XZ_CHECK_CRC64, Crc64Calc (XzCrc64.c:30:
// Crc64Update from CRC64_INIT_VAL ~0, result ^ ~0; reflected polynomial
// kCrc64Poly 0xC96C5795D7870F42, XzCrc64.c:6; byte step CRC64_UPDATE_BYTE,
// XzCrc64.h:16), used by XzCheck_Update / XzCheck_Final (Xz.c:55-85).
//
// GPU formulation (own design): a range of L bytes is cut into chunks of
// kCrcChunk bytes aligned to its END, so only chunk 0 is short.  One lane per
// chunk computes the raw CRC register of its bytes (chunk 0 from the init
// value, the others from 0) with 64 / sizeof(R) slice tables in LDS and aligned
// 16-byte loads (slice-by-16 for 32 bits, two slice-by-8 words for 64); a
// second pass folds the chunk registers of each range:
//     r = shift(r) ^ c_j,   shift(x) = x * x^(8 * kCrcChunk) mod P,
// which is exact because the CRC register is linear over GF(2)
// (R(A||B, init) = shift_|B|(R(A, init)) ^ R(B, 0)).  shift() is a
// table-driven multiply by a constant (sizeof(R) lookups).  Only the 16-byte
// block step and the shift lookup are written per width.
#pragma once

#include <stdint.h>

#include "device_shim.h"

namespace lzgpu {

constexpr uint32_t kCrcChunk = 2048;  // bytes per chunk lane (multiple of 16), both widths
constexpr uint32_t kCrcUnroll = 8;    // aligned 16-byte loads in flight per lane

template <class R>
constexpr R kCrcPoly = R(sizeof(R) == 4 ? 0xEDB88320u : 0xC96C5795D7870F42ull);

// R defaults to CRC-32's register wherever nothing else names the width
template <class R = uint32_t>
struct CrcTables {
  static constexpr uint32_t kSlices = 64 / sizeof(R), kShifts = sizeof(R);
  R slice[kSlices][256];  // slice[k][v]: register after byte v then k zero bytes
  R shift[kShifts][256];  // shift[b][v] = (v << 8b) * x^(8 * kCrcChunk) mod P
};

// a * b mod P in the reflected representation (top bit = x^0)
template <class R>
__host__ __device__ constexpr R crc_mulmod(R a, R b) {
  R p = 0;
  for (R m = R(1) << (8 * sizeof(R) - 1); m != 0; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? ((b >> 1) ^ kCrcPoly<R>) : (b >> 1);
  }
  return p;
}

// x^(8 * nbytes) mod P
template <class R>
__host__ __device__ constexpr R crc_x8n(uint64_t nbytes) {
  R result = R(1) << (8 * sizeof(R) - 1);  // x^0
  R sq = R(1) << (8 * sizeof(R) - 9);      // x^8
  while (nbytes != 0) {
    if (nbytes & 1u) result = crc_mulmod(result, sq);
    sq = crc_mulmod(sq, sq);
    nbytes >>= 1;
  }
  return result;
}

template <class R = uint32_t>
__host__ __device__ constexpr CrcTables<R> crc_make_tables() {
  CrcTables<R> t{};
  for (uint32_t v = 0; v < 256; ++v) {
    R r = v;
    for (int j = 0; j < 8; ++j) r = (r >> 1) ^ ((r & 1u) ? kCrcPoly<R> : R(0));
    t.slice[0][v] = r;
  }
  for (uint32_t k = 1; k < CrcTables<R>::kSlices; ++k)
    for (uint32_t v = 0; v < 256; ++v) {
      const R r = t.slice[k - 1][v];
      t.slice[k][v] = t.slice[0][r & 0xFFu] ^ (r >> 8);
    }
  const R K = crc_x8n<R>(kCrcChunk);
  for (uint32_t b = 0; b < CrcTables<R>::kShifts; ++b)
    for (uint32_t v = 0; v < 256; ++v) t.shift[b][v] = crc_mulmod(K, R(v) << (8 * b));
  return t;
}

// ---------------------------------------------------------------- per-lane code
// a table cell as a lane reads it: LDS on the device
#ifdef LZGPU_HOST_EMU
template <class R>
using crc_cell = const R;
#else
template <class R>
using crc_cell = __attribute__((address_space(3))) const R;
#endif

template <class R>
__device__ __forceinline__ R crc_byte(R crc, uint32_t b, crc_cell<R>* t0) {
  return t0[(crc ^ b) & 0xFFu] ^ (crc >> 8);
}

// bytes [k0, k1) of a 16-byte block, one at a time
template <class R>
__device__ __forceinline__ R crc_block_bytes(R crc, u32x4 v, uint32_t k0, uint32_t k1,
                                             crc_cell<R>* t0) {
  const uint64_t lo = uint64_t(v.x) | (uint64_t(v.y) << 32);
  const uint64_t hi = uint64_t(v.z) | (uint64_t(v.w) << 32);
  for (uint32_t k = k0; k < k1; ++k) {
    const uint32_t b = uint32_t((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)))) & 0xFFu;
    crc = crc_byte<R>(crc, b, t0);
  }
  return crc;
}

// 16 bytes at once, 32 bits: slice[15 - i] for byte i (7zCrc.c's T8 scheme widened to 16)
__device__ __forceinline__ uint32_t crc_block16(uint32_t crc, u32x4 v, crc_cell<uint32_t>* t) {
  const uint32_t x = v.x ^ crc;
  return t[15 * 256 + (x & 0xFFu)] ^ t[14 * 256 + ((x >> 8) & 0xFFu)] ^
         t[13 * 256 + ((x >> 16) & 0xFFu)] ^ t[12 * 256 + (x >> 24)] ^
         t[11 * 256 + (v.y & 0xFFu)] ^ t[10 * 256 + ((v.y >> 8) & 0xFFu)] ^
         t[9 * 256 + ((v.y >> 16) & 0xFFu)] ^ t[8 * 256 + (v.y >> 24)] ^
         t[7 * 256 + (v.z & 0xFFu)] ^ t[6 * 256 + ((v.z >> 8) & 0xFFu)] ^
         t[5 * 256 + ((v.z >> 16) & 0xFFu)] ^ t[4 * 256 + (v.z >> 24)] ^
         t[3 * 256 + (v.w & 0xFFu)] ^ t[2 * 256 + ((v.w >> 8) & 0xFFu)] ^
         t[1 * 256 + ((v.w >> 16) & 0xFFu)] ^ t[0 * 256 + (v.w >> 24)];
}

// 8 bytes (little-endian word w) at once, 64 bits: slice[7 - i] for byte i
__device__ __forceinline__ uint64_t crc_word(uint64_t crc, uint64_t w, crc_cell<uint64_t>* t) {
  const uint64_t x = w ^ crc;
  return t[7 * 256 + (x & 0xFFu)] ^ t[6 * 256 + ((x >> 8) & 0xFFu)] ^
         t[5 * 256 + ((x >> 16) & 0xFFu)] ^ t[4 * 256 + ((x >> 24) & 0xFFu)] ^
         t[3 * 256 + ((x >> 32) & 0xFFu)] ^ t[2 * 256 + ((x >> 40) & 0xFFu)] ^
         t[1 * 256 + ((x >> 48) & 0xFFu)] ^ t[0 * 256 + (x >> 56)];
}

__device__ __forceinline__ uint64_t crc_block16(uint64_t crc, u32x4 v, crc_cell<uint64_t>* t) {
  crc = crc_word(crc, uint64_t(v.x) | (uint64_t(v.y) << 32), t);
  return crc_word(crc, uint64_t(v.z) | (uint64_t(v.w) << 32), t);
}

// shift(r) (sh = CrcTables::shift flattened)
__device__ __forceinline__ uint32_t crc_shift(uint32_t r, crc_cell<uint32_t>* sh) {
  return sh[r & 0xFFu] ^ sh[256 + ((r >> 8) & 0xFFu)] ^ sh[512 + ((r >> 16) & 0xFFu)] ^
         sh[768 + (r >> 24)];
}

__device__ __forceinline__ uint64_t crc_shift(uint64_t r, crc_cell<uint64_t>* sh) {
  uint64_t s = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) s ^= sh[b * 256 + ((r >> (8 * b)) & 0xFFu)];
  return s;
}

// raw CRC register over [p, e) starting from crc (aligned 16-byte loads; an
// aligned block holding a valid byte never crosses a page)
template <class R>
__device__ __forceinline__ R crc_span(R crc, uintptr_t p, uintptr_t e, crc_cell<R>* t) {
  if (p >= e) return crc;
  uintptr_t a = p & ~uintptr_t(15);
  if (a != p || e - a < 16) {
    const uint32_t k1 = e - a < 16 ? uint32_t(e - a) : 16u;
    crc = crc_block_bytes<R>(crc, load16(a), uint32_t(p - a), k1, t);
    a += 16;
  }
  constexpr uint32_t U = kCrcUnroll;
  while (a + 16 * U <= e) {
    u32x4 v[U];
#pragma unroll
    for (uint32_t k = 0; k < U; ++k) v[k] = load16(a + 16 * k);
#pragma unroll
    for (uint32_t k = 0; k < U; ++k) crc = crc_block16(crc, v[k], t);
    a += 16 * U;
  }
  while (a + 16 <= e) {
    crc = crc_block16(crc, load16(a), t);
    a += 16;
  }
  if (a < e) crc = crc_block_bytes<R>(crc, load16(a), 0, uint32_t(e - a), t);
  return crc;
}

// Chunk j of a range of `len` bytes at `base` (chunks end-aligned, chunk 0
// short): its raw register, from `init` for chunk 0 and from 0 otherwise.
// Returns false for a slot beyond the range's chunk count.
template <class R>
__device__ __forceinline__ bool crc_chunk(crc_cell<R>* t, const uint8_t* base, uint64_t len,
                                          uint32_t j, R init, R* out) {
  const uint64_t nch = (len + kCrcChunk - 1) / kCrcChunk;
  if (j >= nch) return false;
  const uint64_t hi = len - (nch - 1 - j) * kCrcChunk;
  const uint64_t lo = j == 0 ? 0 : hi - kCrcChunk;
  const uintptr_t b = (uintptr_t)base;
  *out = crc_span<R>(j == 0 ? init : R(0), b + lo, b + hi, t);
  return true;
}

// Register after the whole range: fold of its chunk registers c[0..nch);
// `init` for an empty range.
template <class R>
__device__ __forceinline__ R crc_fold(crc_cell<R>* sh, const R* c, uint64_t len, R init) {
  const uint32_t nch = uint32_t((len + kCrcChunk - 1) / kCrcChunk);
  if (nch == 0) return init;
  R r = c[0];
  for (uint32_t j = 1; j < nch; ++j) r = crc_shift(r, sh) ^ c[j];
  return r;
}

}  // namespace lzgpu
