// sha256_device.h -- FIPS 180-4 SHA-256 over byte ranges, per-block pieces.
//
// The xz block check XZ_CHECK_SHA256 and the Sha256.h drop-ins (Sha256.c:12-204)
// hash on the device with these pieces; sha256_kernels.hip composes them two
// ways:
//   lane per message   sha256_lane: one lane walks its range block by block
//                      (sha256_message_block, sha256_compress).
//   wave per message   the 64 lanes of a wave take 64 consecutive blocks of one
//                      message.  Half 1, per lane: sha256_message_block +
//                      sha256_schedule, which hands W[t] + K[t] of the lane's
//                      block to a `park` functor (LDS on the device).  Half 2,
//                      wave-uniform: sha256_rounds over the parked blocks in
//                      order, the chaining state carried from block to block.
// A range is padded as the standard says (0x80, zeros, 64-bit big-endian bit
// count) without a byte of it being read or written outside [p, p + len):
// whole blocks load as four 16-byte words, the block that holds the range's
// end is gathered bytewise, and padding blocks past the end read nothing.
//
// Compiles on the host under LZGPU_HOST_EMU (tests/emu_sha256/).
#pragma once

#include <stdint.h>

#include "device_shim.h"

namespace lzgpu {

constexpr uint32_t kSha256Block = 64;  // bytes per compression
// blocks one wave parks per pass of the wave kernel (one per lane)
constexpr uint32_t kSha256Super = 64;

__device__ __forceinline__ void sha256_iv(uint32_t st[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// round constant t; every caller's t is a constant after unrolling
__device__ __forceinline__ uint32_t sha256_k(int t) {
  constexpr uint32_t k[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u,
      0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu,
      0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu,
      0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u,
      0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu,
      0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu,
      0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u,
      0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u,
      0xc67178f2u};
  return k[t];
}

__device__ __forceinline__ uint32_t sha256_rotr(uint32_t x, int r) {
  return (x >> r) | (x << (32 - r));
}
__device__ __forceinline__ uint32_t sha256_bswap(uint32_t x) { return __builtin_bswap32(x); }
// a ^ b ^ c: one v_bitop3_b32 on gfx950 (truth table 0x96), which the compiler
// does not form from two xors by itself
__device__ __forceinline__ uint32_t sha256_xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__gfx950__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  return a ^ b ^ c;
#endif
}

// ---- the big-endian load of one whole 64-byte block
template <class B>
__device__ __forceinline__ void sha256_ld_block(const B* p, uint32_t w[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i)
    w[i] = (uint32_t(p[4 * i]) << 24) | (uint32_t(p[4 * i + 1]) << 16) |
           (uint32_t(p[4 * i + 2]) << 8) | uint32_t(p[4 * i + 3]);
}
// the eight words of a state or digest, as bytes (digest: big-endian words,
// FIPS 180-4 6.2.2; state: the words as the host holds them, little-endian)
template <class B>
__device__ __forceinline__ void sha256_st_words(B* out, const uint32_t st[8], bool digest) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t v = digest ? sha256_bswap(st[i]) : st[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * i + k] = uint8_t(v >> (8 * k));
  }
}
#ifndef LZGPU_HOST_EMU
// global memory runs in unaligned mode (as bcj2_device.h relies on): four
// dwordx4 per block at any byte alignment, one dword store per output word
typedef __attribute__((address_space(1))) uint8_t sha256_gbyte;
typedef uint32_t sha256_u32x4 __attribute__((ext_vector_type(4)));
typedef sha256_u32x4 sha256_u32x4a1 __attribute__((aligned(1)));
typedef uint32_t sha256_u32a1 __attribute__((aligned(1)));
template <>
__device__ __forceinline__ void sha256_ld_block(const sha256_gbyte* p, uint32_t w[16]) {
  const __attribute__((address_space(1))) sha256_u32x4a1* q =
      (const __attribute__((address_space(1))) sha256_u32x4a1*)p;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const sha256_u32x4 v = q[i];
    w[4 * i] = sha256_bswap(v.x);
    w[4 * i + 1] = sha256_bswap(v.y);
    w[4 * i + 2] = sha256_bswap(v.z);
    w[4 * i + 3] = sha256_bswap(v.w);
  }
}
template <>
__device__ __forceinline__ void sha256_st_words(sha256_gbyte* out, const uint32_t st[8],
                                                bool digest) {
  __attribute__((address_space(1))) sha256_u32a1* q =
      (__attribute__((address_space(1))) sha256_u32a1*)out;
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = digest ? sha256_bswap(st[i]) : st[i];
}
#endif

// ---- padding: blocks of the padded message of a range
// compressions a range of len bytes takes: with the padding (0x80 and the
// 8-byte bit count), or its whole blocks only
__device__ __forceinline__ uint64_t sha256_num_blocks(uint64_t len, bool finalise) {
  return finalise ? (len >> 6) + ((len & 63u) >= 56u ? 2u : 1u) : (len >> 6);
}

// Block `blk` of the padded message: the data below len, 0x80 at len, zeros,
// and in the closing block the bit count `bits` of everything hashed (bytes
// before this range included).  Reads only p[0, len).
template <class B>
__device__ __forceinline__ void sha256_message_block(const B* p, uint64_t len, uint64_t bits,
                                                     uint64_t blk, uint32_t w[16]) {
  const uint64_t at = blk * kSha256Block;
  if (at + kSha256Block <= len) {
    sha256_ld_block(p + at, w);
    return;
  }
  // data bytes of this block (0..63; 0 for a block past the 0x80)
  const uint32_t have = at < len ? uint32_t(len - at) : 0u;
  const bool mark = at <= len;  // the 0x80 falls at byte `have` of this block
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t pos = uint32_t(4 * i + k);
      uint32_t b = 0;
      if (pos < have)
        b = uint32_t(p[at + pos]);
      else if (pos == have && mark)
        b = 0x80u;
      v |= b << (24 - 8 * k);
    }
    w[i] = v;
  }
  if (blk + 1 == sha256_num_blocks(len, true)) {
    w[14] = uint32_t(bits >> 32);
    w[15] = uint32_t(bits);
  }
}

// ---- message schedule and compression rounds
__device__ __forceinline__ uint32_t sha256_next_w(uint32_t w[16], int t) {
  if (t >= 16) {
    const uint32_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
    w[t & 15] += sha256_xor3(sha256_rotr(w15, 7), sha256_rotr(w15, 18), w15 >> 3) +
                 w[(t - 7) & 15] +
                 sha256_xor3(sha256_rotr(w2, 17), sha256_rotr(w2, 19), w2 >> 10);
  }
  return w[t & 15];
}

// one round on the working variables v[0..7] = a..h with wk = W[t] + K[t]
__device__ __forceinline__ void sha256_round(uint32_t v[8], uint32_t wk) {
  const uint32_t a = v[0], b = v[1], c = v[2], e = v[4], f = v[5], g = v[6];
  const uint32_t t1 = v[7] + sha256_xor3(sha256_rotr(e, 6), sha256_rotr(e, 11), sha256_rotr(e, 25)) +
                      (g ^ (e & (f ^ g))) + wk;
  const uint32_t t2 = sha256_xor3(sha256_rotr(a, 2), sha256_rotr(a, 13), sha256_rotr(a, 22)) +
                      ((a & b) | (c & (a | b)));
  v[7] = g;
  v[6] = f;
  v[5] = e;
  v[4] = v[3] + t1;
  v[3] = c;
  v[2] = b;
  v[1] = a;
  v[0] = t1 + t2;
}

// The message schedule of one block: park(t, W[t] + K[t]) for t = 0..63
// (w = the block's 16 words, consumed).  Independent of the chaining state.
template <class Park>
__device__ __forceinline__ void sha256_schedule(uint32_t w[16], Park park) {
#pragma unroll
  for (int t = 0; t < 64; ++t) park(t, sha256_next_w(w, t) + sha256_k(t));
}

// The 64 rounds of one block from its parked schedule: wk(t) = W[t] + K[t].
template <class Fetch>
__device__ __forceinline__ void sha256_rounds(uint32_t st[8], Fetch wk) {
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = st[i];
#pragma unroll
  for (int t = 0; t < 64; ++t) sha256_round(v, wk(t));
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] += v[i];
}

// schedule and rounds of one block in one pass (the lane kernel)
__device__ __forceinline__ void sha256_compress(uint32_t st[8], uint32_t w[16]) {
  uint32_t v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = st[i];
#pragma unroll
  for (int t = 0; t < 64; ++t) sha256_round(v, sha256_next_w(w, t) + sha256_k(t));
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] += v[i];
}

// ---- one range on one lane.  st: in = the chaining state to continue from,
// out = the state after the range's blocks (finalise: after its padding, i.e.
// the digest words).  prior = bytes hashed before this range (a multiple of
// 64 when continuing); without finalise the range's len & 63 tail bytes are
// left to the caller.
template <class B>
__device__ __forceinline__ void sha256_lane(const B* p, uint64_t len, uint64_t prior,
                                            bool finalise, uint32_t st[8]) {
  const uint64_t nb = sha256_num_blocks(len, finalise), bits = (prior + len) << 3;
  for (uint64_t blk = 0; blk < nb; ++blk) {
    uint32_t w[16];
    sha256_message_block(p, len, bits, blk, w);
    sha256_compress(st, w);
  }
}

}  // namespace lzgpu
