// lzma2enc_device.h -- the LZMA2 fast-mode encoder for one block: a run of
// LZMA2 chunks that starts with a dictionary reset, on top of
// lzmaenc_device.h's LzmaEnc (match finder, parser, range coder).  A
// restatement of what the reference runs for one block of its multi-threaded
// layout, so that a block's bytes are the reference's:
//
//   driver    MtCallbackImp_Code (Lzma2Enc.c:310-361) without the final 0x00,
//             which belongs to the framing
//   chunk     Lzma2EncInt_EncodeSubblock (:72-164): save the state, encode one
//             chunk, then either an LZMA chunk header in front of the bytes or
//             copy chunks over the same source bytes and the saved state back
//   coder     LzmaEnc_CodeOneMemBlock (LzmaEnc.c:2120-2152) and the useLimits
//             branch of LzmaEnc_CodeOneBlock (:1878-1883)
//   state     LzmaEnc_SaveState / LzmaEnc_RestoreState (:339-389): every
//             probability cell goes to a second table behind the stream's LZMA
//             slice, 16 bytes at a time; `state` and the reps stay in registers
//
// What needs no code here:
//   - LzmaEnc_Init for needInitState.  Until the first LZMA chunk is emitted
//     every attempt ends with the saved state put back, and the state saved
//     before the first attempt is the initial one (lzmaenc_init_slice sets the
//     cells before the lane starts), so the cells, `state` and the reps already
//     hold what LzmaEnc_Init would write;
//   - the range coder's 64 KiB buffer.  A chunk stops once 56 KiB are written
//     (RangeEnc_GetProcessed + 2 * kNumOpts >= 1 << 16), so the reference
//     flushes its buffer once, at the chunk's end, and learns of a short
//     destination only there: it encodes to the same stopping point whatever
//     the capacity, as put_byte's `overflow` does here.
//
// Stores: chunk bytes go to dst + chunk start + header size, bounded by the
// block's remaining capacity (the reference's destLim - *destSize); the header
// is written once the chunk is known.  Every store is below dst_cap.
#pragma once

#include <stddef.h>

#include "lzmaenc_device.h"

namespace lzenc {

constexpr int32_t kErrFail = 11;
constexpr uint32_t kLzma2PackMax = kChunkPackMax, kLzma2UnpackMax = kChunkUnpackMax;
constexpr uint32_t kLzma2CopyChunk = 1u << 16;
constexpr uint32_t kLzma2LcLpMax = 4;

// LzmaEnc's checks plus Lzma2Enc_SetProps' (Lzma2Enc.c:416-417)
LZENC_HD int32_t lzma2_check_params(const Params& q, uint64_t src_len) {
  const int32_t r = check_params(q, src_len);
  if (r != kOk) return r;
  return q.lc + q.lp > kLzma2LcLpMax ? kErrParam : kOk;
}

// Lzma2Enc_WriteProperties (Lzma2Enc.c:423-432)
LZENC_HD uint8_t lzma2_prop_byte(uint32_t dict_size) {
  uint32_t i;
  for (i = 0; i < 40; i++)
    if (dict_size <= ((2u | (i & 1)) << (i / 2 + 11))) break;
  return uint8_t(i);
}

// ---------------------------------------------------------------- props (host side)
// CLzma2EncProps (Lzma2Enc.h:13-19), field for field
struct Enc2Props {
  EncProps lzmaProps;
  size_t blockSize;
  int numBlockThreads;
  int numTotalThreads;
};
constexpr int kNumMtCoderThreadsMax = 32;  // MtCoder.h, a build with threads
// Lzma2EncProps_Init (Lzma2Enc.c:168-174)
LZENC_HD void props2_init(Enc2Props* p) {
  props_init(&p->lzmaProps);
  p->numTotalThreads = -1;
  p->numBlockThreads = -1;
  p->blockSize = 0;
}
// Lzma2EncProps_Normalize (Lzma2Enc.c:176-234)
LZENC_HD void props2_normalize(Enc2Props* p) {
  int t1, t1n, t2, t3;
  {
    EncProps lzmaProps = p->lzmaProps;
    props_normalize(&lzmaProps);
    t1n = lzmaProps.numThreads;
  }
  t1 = p->lzmaProps.numThreads;
  t2 = p->numBlockThreads;
  t3 = p->numTotalThreads;
  if (t2 > kNumMtCoderThreadsMax) t2 = kNumMtCoderThreadsMax;
  if (t3 <= 0) {
    if (t2 <= 0) t2 = 1;
    t3 = t1n * t2;
  } else if (t2 <= 0) {
    t2 = t3 / t1n;
    if (t2 == 0) {
      t1 = 1;
      t2 = t3;
    }
    if (t2 > kNumMtCoderThreadsMax) t2 = kNumMtCoderThreadsMax;
  } else if (t1 <= 0) {
    t1 = t3 / t2;
    if (t1 == 0) t1 = 1;
  } else
    t3 = t1n * t2;
  p->lzmaProps.numThreads = t1;
  p->numBlockThreads = t2;
  p->numTotalThreads = t3;
  props_normalize(&p->lzmaProps);
  if (p->blockSize == 0) {
    const uint32_t dictSize = p->lzmaProps.dictSize;
    uint64_t blockSize = uint64_t(dictSize) << 2;
    const uint32_t kMinSize = 1u << 20, kMaxSize = 1u << 28;
    if (blockSize < kMinSize) blockSize = kMinSize;
    if (blockSize > kMaxSize) blockSize = kMaxSize;
    if (blockSize < dictSize) blockSize = dictSize;
    p->blockSize = size_t(blockSize);
  }
}
// Lzma2Enc_SetProps' check (Lzma2Enc.c:411-421), then Lzma2EncInt_Init's
// LzmaEnc_SetProps as params_from_props states it.  q and prop are written
// only on SZ_OK; prop is Lzma2Enc_WriteProperties' byte.
// `allowed` and `field` as params_from_props_ex's.
LZENC_HD int32_t lzma2_params_from_props_ex(const Enc2Props* props, uint32_t allowed, Params* q,
                                            uint8_t* prop, const char** field = nullptr) {
  EncProps lzmaProps = props->lzmaProps;
  props_normalize(&lzmaProps);
  if (lzmaProps.lc + lzmaProps.lp > int(kLzma2LcLpMax)) return kErrParam;
  Enc2Props n = *props;
  props2_normalize(&n);
  Params t;
  const int32_t r = params_from_props_ex(&n.lzmaProps, 0, allowed, &t, field);
  if (r != kOk) return r;
  *q = t;
  *prop = lzma2_prop_byte(t.dict_size);
  return kOk;
}
LZENC_HD int32_t lzma2_params_from_props(const Enc2Props* props, Params* q, uint8_t* prop) {
  return lzma2_params_from_props_ex(props, 0, q, prop);
}

// One block's slice: the LZMA slice, then the saved probability table
// (`saved_bytes`, the cells rounded up to 16 bytes).  `bytes` is a multiple
// of 256.
struct Layout2 {
  Layout l;
  uint64_t saved, saved_bytes, bytes;
};
LZENC_HD Layout2 lzma2enc_layout(const Params& q, uint64_t src_len) {
  Layout2 m;
  m.l = lzmaenc_layout(q, src_len);
  m.saved = m.l.bytes;
  m.saved_bytes = m.l.matches;
  m.bytes = (m.saved + m.saved_bytes + 255) & ~uint64_t(255);
  return m;
}

// n bytes, a multiple of 16, between two 16-byte aligned tables
LZENC_FN void copy16(uint8_t* to, const uint8_t* from, uint64_t n) {
  struct alignas(16) V16 {
    uint32_t w[4];
  };
  for (uint64_t i = 0; i < n; i += 16) {
    V16 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(from + i, 16), 16);
    __builtin_memcpy(__builtin_assume_aligned(to + i, 16), &v, 16);
  }
}

// kNormal as LzmaEncT's: false is the fast path alone, true the reference's
// encoder with its two mode bits at run time.
template <bool kNormal>
struct Lzma2EncT : LzmaEncT<kNormal> {
  using B = LzmaEncT<kNormal>;
  using B::additionalOffset;
  using B::cache;
  using B::cacheSize;
  using B::crc;
  using B::cutValue;
  using B::cyclicBufferPos;
  using B::cyclicBufferSize;
  using B::dst;
  using B::dst_cap;
  using B::finished;
  using B::hash;
  using B::hashMask;
  using B::lc;
  using B::longestMatchLength;
  using B::low;
  using B::lpMask;
  using B::matches;
  using B::nowPos64;
  using B::numAvail;
  using B::numFastBytes;
  using B::numPairs;
  using B::off;
  using B::outPos;
  using B::overflow;
  using B::pbMask;
  using B::probs;
  using B::range;
  using B::rep0;
  using B::rep1;
  using B::rep2;
  using B::rep3;
  using B::son;
  using B::src;
  using B::src_len;
  using B::state;
  using B::writeEndMark;

  using B::avail;
  using B::flush;
  using B::read_match_distances;
  using B::encode_bit;
  using B::lit_next;
  using B::lit_encode;
  using B::get_optimum_fast;
  using B::lit_encode_matched;
  using B::rep;
  using B::short_rep_next;
  using B::len_encode;
  using B::rep_next;
  using B::match_next;
  using B::get_pos_slot;
  using B::tree_encode;
  using B::len_to_pos_state;
  using B::tree_reverse_encode;
  using B::encode_direct_bits;

  // LzmaEnc_CodeOneBlock(p, True, 1 << 16, 1 << 21).  The normal modes take
  // LzmaEncT's code_block<true>; the fast path keeps its own text of
  // code_one_block with the chunk limits in place of the 32 KiB progress step,
  // always ending in Flush (the token coding in the middle is the same text),
  // so that its kernel stays the code it was.
  LZENC_FN void code_chunk() {
    if constexpr (kNormal) {
      this->template code_block<true>();
    } else {
      uint32_t nowPos32 = nowPos64;
      const uint32_t startPos32 = nowPos32;

      if (nowPos64 == 0) {
        uint32_t pairs;
        if (avail() == 0) {
          flush(nowPos32);
          return;
        }
        read_match_distances(&pairs);
        encode_bit(kIsMatch + state * 16, 0);
        state = lit_next(state);
        const uint32_t curByte = src[off - additionalOffset];
        lit_encode(kLit, curByte);
        additionalOffset--;
        nowPos32++;
      }

      if (avail() != 0)
        for (;;) {
          uint32_t pos;
          const uint32_t len = get_optimum_fast(&pos);
          const uint32_t posState = nowPos32 & pbMask;
          if (len == 1 && pos == 0xFFFFFFFFu) {
            encode_bit(kIsMatch + state * 16 + posState, 0);
            const uint8_t* data = src + off - additionalOffset;
            const uint32_t curByte = *data;
            const uint32_t lit =
                kLit + (((nowPos32 & lpMask) << lc) + (uint32_t(*(data - 1)) >> (8 - lc))) * 0x300;
            if (state < 7)
              lit_encode(lit, curByte);
            else
              lit_encode_matched(lit, curByte, *(data - rep0 - 1));
            state = lit_next(state);
          } else {
            encode_bit(kIsMatch + state * 16 + posState, 1);
            if (pos < kNumReps) {
              encode_bit(kIsRep + state, 1);
              if (pos == 0) {
                encode_bit(kIsRepG0 + state, 0);
                encode_bit(kIsRep0Long + state * 16 + posState, (len == 1) ? 0 : 1);
              } else {
                const uint32_t distance = rep(pos);
                encode_bit(kIsRepG0 + state, 1);
                if (pos == 1)
                  encode_bit(kIsRepG1 + state, 0);
                else {
                  encode_bit(kIsRepG1 + state, 1);
                  encode_bit(kIsRepG2 + state, pos - 2);
                  if (pos == 3) rep3 = rep2;
                  rep2 = rep1;
                }
                rep1 = rep0;
                rep0 = distance;
              }
              if (len == 1)
                state = short_rep_next(state);
              else {
                len_encode(kRepLenEnc, len - kMatchLenMin, posState);
                state = rep_next(state);
              }
            } else {
              encode_bit(kIsRep + state, 0);
              state = match_next(state);
              len_encode(kLenEnc, len - kMatchLenMin, posState);
              pos -= kNumReps;
              const uint32_t posSlot = get_pos_slot(pos);
              tree_encode(kPosSlot + len_to_pos_state(len) * 64, 6, posSlot);
              if (posSlot >= kStartPosModelIndex) {
                const uint32_t footerBits = (posSlot >> 1) - 1;
                const uint32_t base = (2 | (posSlot & 1)) << footerBits;
                const uint32_t posReduced = pos - base;
                if (posSlot < kEndPosModelIndex)
                  tree_reverse_encode(kPosEncoders + base - posSlot - 1, int(footerBits), posReduced);
                else {
                  encode_direct_bits(posReduced >> kNumAlignBits, int(footerBits - kNumAlignBits));
                  tree_reverse_encode(kPosAlign, kNumAlignBits, posReduced & 15);
                }
              }
              rep3 = rep2;
              rep2 = rep1;
              rep1 = rep0;
              rep0 = pos;
            }
          }
          additionalOffset -= len;
          nowPos32 += len;
          if (additionalOffset == 0) {
            if (avail() == 0) break;
            const uint32_t processed = nowPos32 - startPos32;
            // RangeEnc_GetProcessed: the chunk's bytes written plus cacheSize
            if (processed + kNumOpts + 300 >= kLzma2UnpackMax ||
                outPos + cacheSize + kNumOpts * 2 >= kLzma2PackMax)
              break;
          }
        }
      nowPos64 += nowPos32 - startPos32;
      flush(nowPos32);
    
    }
  }


  // One block: q has passed lzma2_check_params, the slice lzmaenc_init_slice.
  // {SZ_OK, bytes of all chunks} or {SZ_ERROR_OUTPUT_EOF, bytes of the whole
  // chunks before the one that did not fit} (*destSize when MtCallbackImp_Code
  // breaks); bytes in [dest_len, dst_cap_) are then unspecified.
  LZENC_FN Out encode_block(const uint8_t* src_, uint32_t src_len_, uint8_t* dst_,
                            uint64_t dst_cap_, const Params& q, uint8_t* slice, const Layout2& m,
                            const uint32_t* crc_, const uint32_t* probPrices_ = nullptr) {
    src = src_;
    probs = reinterpret_cast<uint16_t*>(slice + m.l.probs);
    matches = reinterpret_cast<uint32_t*>(slice + m.l.matches);
    hash = reinterpret_cast<uint32_t*>(slice + m.l.hash);
    son = reinterpret_cast<uint32_t*>(slice + m.l.son);
    crc = crc_;
    src_len = src_len_;
    lc = q.lc;
    lpMask = (1u << q.lp) - 1;
    pbMask = (1u << q.pb) - 1;
    numFastBytes = q.fb;
    cutValue = q.mc;
    writeEndMark = 0;
    hashMask = hash_mask(q.dict_size);
    cyclicBufferSize = q.dict_size + 1;
    // MatchFinder_Init, LzmaEnc_Init
    off = 0;
    cyclicBufferPos = 0;
    state = 0;
    rep0 = rep1 = rep2 = rep3 = 0;
    additionalOffset = 0;
    longestMatchLength = numPairs = numAvail = 0;
    nowPos64 = 0;
    if constexpr (kNormal) this->setup_normal(q, slice, m.l, probPrices_);
    // Lzma2EncInt_Init
    const uint8_t lzmaProps = uint8_t((q.pb * 5 + q.lp) * 9 + q.lc);
    uint8_t* const cells = slice + m.l.probs;
    uint8_t* const saved = slice + m.saved;
    uint32_t srcPos = 0;
    bool needInitState = true, needInitProp = true;
    Out o;
    o.res = kOk;
    o.dest_len = 0;

    while (srcPos < src_len) {
      // Lzma2EncInt_EncodeSubblock(p, dest + *destSize, &packSize, NULL)
      uint8_t* const outBuf = dst_ + o.dest_len;
      const uint64_t packSizeLimit = dst_cap_ - o.dest_len;
      const uint32_t lzHeaderSize = 5 + (needInitProp ? 1 : 0);
      if (packSizeLimit < lzHeaderSize) {
        o.res = kErrOutputEof;
        break;
      }
      // LzmaEnc_SaveState
#ifndef LZMA2ENC_AB_NO_SAVE  // A/B builds only: times the save; wrong after a copy chunk
      copy16(saved, cells, m.saved_bytes);
#endif
      const uint32_t s_state = state, s_rep0 = rep0, s_rep1 = rep1, s_rep2 = rep2, s_rep3 = rep3;
      // LzmaEnc_CodeOneMemBlock
      dst = outBuf + lzHeaderSize;
      dst_cap = packSizeLimit - lzHeaderSize;
      outPos = 0;
      overflow = 0;
      finished = 0;
      low = 0;
      range = 0xFFFFFFFFu;
      cacheSize = 1;
      cache = 0;
      // LzmaEnc_InitPrices (LzmaEnc.c:2139): every price table is rebuilt from
      // the cells, so cells, reps and state are all a restore has to put back
      if constexpr (kNormal) this->init_prices();
      const uint32_t before = nowPos64;
      code_chunk();
      uint32_t unpackSize = nowPos64 - before;
      const uint64_t packSize = overflow ? dst_cap : outPos;
      if (unpackSize == 0) {  // not reached: srcPos < src_len leaves input to code
        o.res = kErrFail;
        break;
      }
      if (overflow || packSize + 2 >= unpackSize || packSize > kLzma2PackMax) {
        uint64_t destPos = 0;
        const uint8_t* from = src + off - additionalOffset - unpackSize;  // LzmaEnc_GetCurBuf
        bool fits = true;
        while (unpackSize > 0) {
          const uint32_t u = unpackSize < kLzma2CopyChunk ? unpackSize : kLzma2CopyChunk;
          if (packSizeLimit - destPos < uint64_t(u) + 3) {
            fits = false;
            break;
          }
          outBuf[destPos++] = uint8_t(srcPos == 0 ? 1 : 2);
          outBuf[destPos++] = uint8_t((u - 1) >> 8);
          outBuf[destPos++] = uint8_t(u - 1);
          for (uint32_t i = 0; i < u; ++i) outBuf[destPos + i] = from[i];
          from += u;
          unpackSize -= u;
          destPos += u;
          srcPos += u;
        }
        if (!fits) {
          o.res = kErrOutputEof;
          break;
        }
        // LzmaEnc_RestoreState; the match finder and nowPos64 stay advanced
        copy16(cells, saved, m.saved_bytes);
        state = s_state;
        rep0 = s_rep0;
        rep1 = s_rep1;
        rep2 = s_rep2;
        rep3 = s_rep3;
        o.dest_len += destPos;
      } else {
        const uint32_t u = unpackSize - 1;
        const uint32_t pm = uint32_t(packSize - 1);
        const uint32_t mode = srcPos == 0 ? 3 : needInitState ? (needInitProp ? 2 : 1) : 0;
        outBuf[0] = uint8_t(0x80 | (mode << 5) | ((u >> 16) & 0x1F));
        outBuf[1] = uint8_t(u >> 8);
        outBuf[2] = uint8_t(u);
        outBuf[3] = uint8_t(pm >> 8);
        outBuf[4] = uint8_t(pm);
        if (needInitProp) outBuf[5] = lzmaProps;
        needInitProp = false;
        needInitState = false;
        o.dest_len += lzHeaderSize + packSize;
        srcPos += unpackSize;
      }
    }
    return o;
  }
};
using Lzma2Enc = Lzma2EncT<false>;
using Lzma2EncNormal = Lzma2EncT<true>;

}  // namespace lzenc
