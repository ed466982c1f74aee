// lzmaenc_device.h -- the LZMA fast-mode encoder for one stream: hash-chain
// match finder, greedy parser and range coder, as one struct whose scalar state
// is meant to live in registers.  A restatement of exactly what the reference's
// LzmaEncode executes when the normalised props have algo == 0 and btMode == 0
// (levels 0..4, LzmaEnc.c:53-74), so the output is the reference's, bit for bit:
//
//   match finder  Hc4_MatchFinder_GetMatches (LzFind.c:586-633),
//                 Hc4_MatchFinder_Skip (:704-719), Hc_GetMatchesSpec (:322-351),
//                 HASH4_CALC (LzHash.h:22-26), the geometry of MatchFinder_Create
//                 (:191-229) and MatchFinder_Init (:271-283), in direct-input
//                 mode (LzmaEnc.c:2057-2062, LzFind.c:61-71): the source buffer
//                 is the window, nothing is copied or moved
//   parser        ReadMatchDistances (LzmaEnc.c:816-849), MovePos (:803-814),
//                 GetOptimumFast with ChangePair (:1487-1595)
//   coder         LzmaEnc_CodeOneBlock (:1733-1893) driven as LzmaEnc_Encode2
//                 drives it (:2154-2182), Flush / WriteEndMarker (:1597-1632),
//                 LzmaEnc_Init (:1947-2003), the range encoder (:483-573) and
//                 the tree / literal / length coders (:575-598, :666-691, :733-754)
//   output        MyWrite (:2093-2105): what fits is written, the rest sets
//                 `overflow`; the outcome is then SZ_ERROR_OUTPUT_EOF with
//                 dest_len == dst_cap and dst holding the first dst_cap bytes of
//                 the full stream
//
// Differences from the reference, all without effect on a byte of output:
//   - no normalisation of positions (MatchFinder_Normalize): a source of 2^31
//     bytes or more is SZ_ERROR_UNSUPPORTED, which keeps pos = dictSize + 1 +
//     offset below kMaxValForNormalize for every dictionary up to 1 << 30;
//   - lenLimit is min(numFastBytes, bytes left) at every position.  The
//     reference caches it between MatchFinder_SetLimits calls (LzFind.c:246-269)
//     but sets posLimit so that the cached value equals this one;
//   - the ring position wraps as soon as it reaches cyclicBufferSize; the
//     reference wraps in MatchFinder_CheckLimits (:317-318), which its posLimit
//     reaches at the same position;
//   - GetPosSlot is computed from the highest set bit, for every 32-bit
//     distance (the reference's g_FastPos table covers what a 1 << 30
//     dictionary can produce);
//   - bytes go straight to dst; the reference collects them in a 64 KiB buffer
//     and notices an overflow at the next buffer flush, this code at the byte
//     that does not fit.  Both stop at the next CheckErrors (block start, block
//     end, Flush), and bytes below dst_cap are final once written, so dst and
//     dest_len are the same;
//   - cacheSize is 32 bits wide (it is bounded by the output length < 2^32);
//   - the price tables of the optimal parser are never built: the fast path
//     reads none (LenEnc_Encode2 is called with updatePrice == !fastMode,
//     LzmaEnc.c:1827,1836, and :1868-1874 is skipped).
//
// The normal modes (LzmaEncT<true>: algo == 1 and / or btMode == 1 with
// numHashBytes 4, levels 5..9) add, restated the same way: the finder
// Bt4_MatchFinder_GetMatches / _Skip with GetMatchesSpec1 and SkipMatchesSpec
// (LzFind.c:353-456, :539-584, :688-702); the price tables (LzmaEnc.c:600-798,
// :1634-1674, :2005-2018) with the refresh of :1865-1874; GetOptimum and
// Backward (:856-1485).  There LenEnc_Encode2 counts down and rebuilds the
// length prices as the reference does.  The output is that of the reference's
// single-threaded encoder (_7ZIP_ST).
//
// Memory of one stream (lzmaenc_layout): the probability cells, the `matches`
// array, the hash (kFix4HashSize fixed entries + hashMask + 1) and the `son`
// ring.  The hash must be all zero and the cells kProbInit before
// LzmaEnc::encode runs (lzmaenc_init_slice, dealt over the whole grid on the
// device); `matches` and `son` need no initialisation: every entry read was
// written before, as in the reference, which does not clear `son` either.
//
// Bounds: every source index is below src_len (match candidates are positions
// the finder itself inserted, so delta <= offset; the guards `delta <= off`
// below are implied by `delta < cyclicBufferSize` and only keep a corrupted
// hash from steering a read outside the source), every store to dst is below
// dst_cap, and the ring index is below son_entries.
#pragma once

#include <stdint.h>

#ifdef LZGPU_HOST_EMU
#define LZENC_FN inline
#define LZENC_HD inline
#else
#include <hip/hip_runtime.h>
#define LZENC_FN __device__ __forceinline__
#define LZENC_HD __host__ __device__ inline
#endif
// The normal-mode kernels' translation units define LZENC_DEVICE_NOINLINE, which
// makes ReadMatchDistances a real call there: see lzmaenc_normal_kernels.hip.
#if !defined(LZGPU_HOST_EMU) && defined(LZENC_DEVICE_NOINLINE)
#define LZENC_FN_RMD __device__ __noinline__
#else
#define LZENC_FN_RMD LZENC_FN
#endif

namespace lzenc {

constexpr int32_t kOk = 0, kErrUnsupported = 4, kErrParam = 5, kErrOutputEof = 7;

constexpr uint32_t kNumStates = 12, kNumReps = 4;
constexpr uint32_t kMatchLenMin = 2, kMatchLenMax = 273;
constexpr uint32_t kProbInit = 1024;
constexpr uint32_t kTopValue = 1u << 24;
constexpr uint32_t kStartPosModelIndex = 4, kEndPosModelIndex = 14, kNumAlignBits = 4;
constexpr uint32_t kHash2Size = 1u << 10, kHash3Size = 1u << 16;
constexpr uint32_t kFix3HashSize = kHash2Size, kFix4HashSize = kHash2Size + kHash3Size;
constexpr uint32_t kDictMax = 1u << 30;  // kDicLogSizeMaxCompress of a 64-bit build

// probability cells (16-bit), fixed sections first, literals last
constexpr uint32_t kIsMatch = 0;                         // [12][16]
constexpr uint32_t kIsRep = kIsMatch + kNumStates * 16;  // [12]
constexpr uint32_t kIsRepG0 = kIsRep + kNumStates;
constexpr uint32_t kIsRepG1 = kIsRepG0 + kNumStates;
constexpr uint32_t kIsRepG2 = kIsRepG1 + kNumStates;
constexpr uint32_t kIsRep0Long = kIsRepG2 + kNumStates;      // [12][16]
constexpr uint32_t kPosSlot = kIsRep0Long + kNumStates * 16;  // [4][64]
constexpr uint32_t kPosEncoders = kPosSlot + 4 * 64;          // [128 - 14]
constexpr uint32_t kPosAlign = kPosEncoders + 128 - kEndPosModelIndex;  // [16]
constexpr uint32_t kLenEnc = kPosAlign + 16;   // choice, choice2, low[128], mid[128], high[256]
constexpr uint32_t kLenCells = 2 + 128 + 128 + 256;
constexpr uint32_t kRepLenEnc = kLenEnc + kLenCells;
constexpr uint32_t kLit = kRepLenEnc + kLenCells;
constexpr uint32_t kLenLow = 2, kLenMid = 2 + 128, kLenHigh = 2 + 256;

// room for the reference's matches[LZMA_MATCH_LEN_MAX * 2 + 2 + 1]
constexpr uint32_t kMatchesWords = 552;

// algo: 1 = the optimal parser (GetOptimum), 0 = the fast one; bt: 1 = the
// binary-tree finder Bt4, 0 = the hash chains Hc4.  Both 0 is the fast path.
struct Params {
  uint32_t dict_size, lc, lp, pb, fb, mc, write_end_mark;
  uint32_t algo = 0, bt = 0;
};
constexpr uint32_t kModeOptimal = 1, kModeBt4 = 2;
LZENC_HD uint32_t mode_of(const Params& q) {
  return (q.algo ? kModeOptimal : 0u) | (q.bt ? kModeBt4 : 0u);
}

// SZ_OK, or what the stream ends with before anything is read or written
LZENC_HD int32_t check_params(const Params& q, uint64_t src_len) {
  if (q.lc > 8 || q.lp > 4 || q.pb > 4 || q.dict_size == 0 || q.dict_size > kDictMax ||
      q.fb < 5 || q.fb > kMatchLenMax || q.algo > 1 || q.bt > 1)
    return kErrParam;
  if (src_len >= (uint64_t(1) << 31)) return kErrUnsupported;
  return kOk;
}

// Encoder sessions (LzmaEncT<false>::session_call).  A call that is not the
// last starts a token only while this many supplied bytes lie ahead of it.
constexpr uint32_t kSessionHold = 2 * kMatchLenMax;
constexpr int32_t kSessionNeedsInput = 0, kSessionFinished = 1, kSessionBudget = 2;
// what a call ends a session with before touching memory: the props, the
// append-only source (src_len within src_cap, never behind what is encoded),
// the slice's alignment
template <class S>
LZENC_HD Params session_params(const S& s) {
  Params q;
  q.dict_size = s.dict_size;
  q.lc = s.lc;
  q.lp = s.lp;
  q.pb = s.pb;
  q.fb = s.fb;
  q.mc = s.mc;
  q.write_end_mark = s.write_end_mark;
  return q;
}
template <class S>
LZENC_HD int32_t session_check(const S& s) {
  const int32_t r = check_params(session_params(s), s.src_cap);
  if (r != kOk) return r;
  if (s.src_len > s.src_cap || s.src_len < s.in_pos) return kErrParam;
  return (uint64_t(reinterpret_cast<uintptr_t>(s.ws)) & 15u) ? kErrParam : kOk;
}
// whether a round has anything to do for the session: the list pass's test.  A
// record session_check refuses has work once: the lane that ends it.
template <class S>
LZENC_HD bool session_has_work(const S& s, uint32_t hold) {
  if (s.finished) return false;
  if (session_check(s) != kOk) return true;
  return s.finish != 0 || s.src_len - s.in_pos >= hold;
}
// and whether the round has to initialise its slice first
template <class S>
LZENC_HD bool session_wants_init(const S& s, uint32_t hold) {
  return s.needs_init != 0 && session_has_work(s, hold) && session_check(s) == kOk;
}

// MatchFinder_Create's hashMask for numHashBytes == 4 (LzFind.c:200-215)
LZENC_HD uint32_t hash_mask(uint32_t dict_size) {
  uint32_t hs = dict_size - 1;
  hs |= hs >> 1;
  hs |= hs >> 2;
  hs |= hs >> 4;
  hs |= hs >> 8;
  hs >>= 1;
  hs |= 0xFFFF;
  if (hs > (1u << 24)) hs >>= 1;
  return hs;
}

// One stream's slice of the workspace, offsets in bytes from the slice start
// (each a multiple of 16), `bytes` a multiple of 256.
// The optimal parser adds `prices` (price_words 32-bit words: the two length
// price tables of 1 << pb position states, their counters, the slot, distance
// and align prices and FillDistancesPrices' tempPrices) and `opt` (kNumOpts
// cells); Bt4 doubles `son` (two words per ring slot).  A mode that has no use
// for a region gets none.
struct Layout {
  uint64_t probs, matches, hash, son, bytes;
  uint32_t prob_cells, hash_words, son_entries;
  uint64_t prices, opt;
  uint32_t price_words;
};
constexpr uint32_t kNumOpts = 1u << 12;
// LZMA2's chunk limits (Lzma2Enc.c: LZMA2_PACK_SIZE_MAX, LZMA2_UNPACK_SIZE_MAX)
constexpr uint32_t kChunkPackMax = 1u << 16, kChunkUnpackMax = 1u << 21;
// COptimal (LzmaEnc.c:142-156), field for field: 48 bytes
struct Opt {
  uint32_t price, state, prev1IsChar, prev2, posPrev2, backPrev2, posPrev, backPrev, backs[4];
};
constexpr uint32_t kLenSymbols = 272;  // kLenNumSymbolsTotal
constexpr uint32_t kNumFullDistances = 128, kAlignTableSize = 16;
// words of the `prices` region after the 2 << pb length tables
constexpr uint32_t kPrLenCounters = 0;                    // [2][16]
constexpr uint32_t kPrPosSlot = kPrLenCounters + 32;      // [4][64]
constexpr uint32_t kPrDistances = kPrPosSlot + 4 * 64;    // [4][128]
constexpr uint32_t kPrAlign = kPrDistances + 4 * kNumFullDistances;  // [16]
constexpr uint32_t kPrTemp = kPrAlign + kAlignTableSize;  // [128]
constexpr uint32_t kPrFixedWords = kPrTemp + kNumFullDistances;
LZENC_HD Layout lzmaenc_layout(const Params& q, uint64_t src_len) {
  Layout l;
  l.prob_cells = kLit + (0x300u << (q.lc + q.lp));
  l.hash_words = kFix4HashSize + hash_mask(q.dict_size) + 1;
  // a stream no longer than its dictionary never wraps the ring
  l.son_entries = uint32_t(src_len < q.dict_size ? src_len : q.dict_size) + 1;
  if (q.bt) l.son_entries *= 2;
  l.probs = 0;
  l.matches = (uint64_t(l.prob_cells) * 2 + 15) & ~uint64_t(15);
  l.hash = l.matches + kMatchesWords * 4;
  l.son = l.hash + uint64_t(l.hash_words) * 4;
  uint64_t end = l.son + uint64_t(l.son_entries) * 4;
  l.prices = l.opt = 0;
  l.price_words = 0;
  if (q.algo) {
    l.price_words = (2u << q.pb) * kLenSymbols + kPrFixedWords;
    l.prices = (end + 15) & ~uint64_t(15);
    l.opt = l.prices + uint64_t(l.price_words) * 4;
    end = l.opt + uint64_t(kNumOpts) * sizeof(Opt);
  }
  l.bytes = (end + 255) & ~uint64_t(255);
  return l;
}

// ---------------------------------------------------------------- props (host side)
// CLzmaEncProps (LzmaEnc.h:15-31), field for field
struct EncProps {
  int level;
  uint32_t dictSize;
  int lc, lp, pb, algo, fb, btMode, numHashBytes;
  uint32_t mc;
  unsigned writeEndMark;
  int numThreads;
};
// LzmaEncProps_Init (LzmaEnc.c:45-51)
LZENC_HD void props_init(EncProps* p) {
  p->level = 5;
  p->dictSize = p->mc = 0;
  p->lc = p->lp = p->pb = p->algo = p->fb = p->btMode = p->numHashBytes = p->numThreads = -1;
  p->writeEndMark = 0;
}
// LzmaEncProps_Normalize (LzmaEnc.c:53-74) of a build with threads (no _7ZIP_ST)
LZENC_HD void props_normalize(EncProps* p) {
  int level = p->level;
  if (level < 0) level = 5;
  p->level = level;
  if (p->dictSize == 0)
    p->dictSize = (level <= 5 ? (1u << (level * 2 + 14)) : (level == 6 ? (1u << 25) : (1u << 26)));
  if (p->lc < 0) p->lc = 3;
  if (p->lp < 0) p->lp = 0;
  if (p->pb < 0) p->pb = 2;
  if (p->algo < 0) p->algo = (level < 5 ? 0 : 1);
  if (p->fb < 0) p->fb = (level < 7 ? 32 : 64);
  if (p->btMode < 0) p->btMode = (p->algo == 0 ? 0 : 1);
  if (p->numHashBytes < 0) p->numHashBytes = 4;
  if (p->mc == 0) p->mc = (16 + (uint32_t(p->fb) >> 1)) >> (p->btMode ? 0 : 1);
  if (p->numThreads < 0) p->numThreads = ((p->btMode && p->algo) ? 2 : 1);
}
// LzmaEnc_SetProps' checks and clamps (LzmaEnc.c:391-443) into the encoder's
// parameters: SZ_ERROR_PARAM as there, then SZ_ERROR_UNSUPPORTED for what
// `allowed` (kModeOptimal | kModeBt4) does not admit: algo != 0 without
// kModeOptimal, btMode != 0 without kModeBt4, and btMode != 0 with
// numHashBytes below 4 (Bt2 / Bt3) always.  *field then names the props field.
// q is written only on SZ_OK.
LZENC_HD int32_t params_from_props_ex(const EncProps* props2, int writeEndMark, uint32_t allowed,
                                      Params* q, const char** field = nullptr) {
  EncProps props = *props2;
  props_normalize(&props);
  if (props.lc > 8 || props.lp > 4 || props.pb > 4 || props.dictSize > kDictMax) return kErrParam;
  const char* why = nullptr;
  if (props.algo != 0 && !(allowed & kModeOptimal)) why = "algo";
  if (props.btMode != 0 && !(allowed & kModeBt4)) why = why ? "algo and btMode" : "btMode";
  if (props.btMode != 0 && props.numHashBytes < 4) why = "numHashBytes";
  if (why) {
    if (field) *field = why;
    return kErrUnsupported;
  }
  uint32_t fb = uint32_t(props.fb);
  if (fb < 5) fb = 5;
  if (fb > kMatchLenMax) fb = kMatchLenMax;
  q->dict_size = props.dictSize;
  q->lc = uint32_t(props.lc);
  q->lp = uint32_t(props.lp);
  q->pb = uint32_t(props.pb);
  q->fb = fb;
  q->mc = props.mc;
  q->write_end_mark = writeEndMark ? 1u : 0u;
  q->algo = props.algo != 0 ? 1u : 0u;
  q->bt = props.btMode != 0 ? 1u : 0u;
  return kOk;
}
// the fast path alone: SZ_ERROR_UNSUPPORTED for algo != 0 or btMode != 0
LZENC_HD int32_t params_from_props(const EncProps* props2, int writeEndMark, Params* q) {
  return params_from_props_ex(props2, writeEndMark, 0, q);
}
// LzmaEnc_WriteProperties (LzmaEnc.c:2191-2218): the dictionary size is
// rounded up to 2^n or 3 * 2^(n-1) in the header only
LZENC_HD void write_props5(const Params& q, uint8_t* props5) {
  uint32_t dictSize = q.dict_size;
  props5[0] = uint8_t((q.pb * 5 + q.lp) * 9 + q.lc);
  for (int i = 11; i <= 30; i++) {
    if (dictSize <= (2u << i)) {
      dictSize = (2u << i);
      break;
    }
    if (dictSize <= (3u << i)) {
      dictSize = (3u << i);
      break;
    }
  }
  for (int i = 0; i < 4; i++) props5[1 + i] = uint8_t(dictSize >> (8 * i));
}

// p->crc[] of the match finder (LzFind.c:141-148): the project's CRC-32 table
// (slice 0 of crc_device.h's CrcTables<uint32_t>, polynomial 0xEDB88320), entry v
LZENC_HD uint32_t crc_entry(uint32_t v) {
  uint32_t r = v;
  for (int j = 0; j < 8; ++j) r = (r >> 1) ^ ((r & 1u) ? 0xEDB88320u : 0u);
  return r;
}

struct Out {
  int32_t res;
  uint64_t dest_len;
};

// LzmaEnc_InitPriceTables (LzmaEnc.c:600-621): entry i of ProbPrices[128], the
// same for every stream
LZENC_HD uint32_t prob_price_entry(uint32_t i) {
  uint32_t w = (i << 4) + 8, bitCount = 0;
  for (int j = 0; j < 4; j++) {
    w = w * w;
    bitCount <<= 1;
    while (w >= (1u << 16)) {
      w >>= 1;
      bitCount++;
    }
  }
  return (11u << 4) - 15 - bitCount;
}
constexpr uint32_t kProbPricesWords = 128;
constexpr uint32_t kInfinityPrice = 1u << 30;

// kNormal == false is the fast path alone (Hc4 and GetOptimumFast; every
// `if constexpr (kNormal)` below drops out and the price members are never
// touched).  kNormal == true is the reference's encoder with its two mode bits
// at run time: fastMode (GetOptimumFast or GetOptimum) and btMode (Hc4 or Bt4).
template <bool kNormal>
struct LzmaEncT {
  // memory
  const uint8_t* src;
  uint8_t* dst;
  uint16_t* probs;
  uint32_t* matches;
  uint32_t* hash;
  uint32_t* son;
  const uint32_t* crc;
  // normal mode: the price tables and the opt array of the slice, ProbPrices,
  // and the reference's price bookkeeping
  uint32_t* lenPrices;  // [2][1 << pb][kLenSymbols]: lenEnc, then repLenEnc
  uint32_t* prFixed;    // kPr* words
  Opt* opt;
  const uint32_t* probPrices;
  uint32_t fastMode, btMode, pbBits, lenTableSize, distTableSize;
  uint32_t alignPriceCount, matchPriceCount, optimumEndIndex, optimumCurrentIndex;
  // props
  uint32_t src_len, lc, lpMask, pbMask, numFastBytes, cutValue, writeEndMark;
  uint32_t hashMask, cyclicBufferSize;
  uint64_t dst_cap;
  // match finder: off = buffer - bufferBase; pos = cyclicBufferSize + off
  uint32_t off, cyclicBufferPos;
  // parser
  uint32_t longestMatchLength, numPairs, numAvail, additionalOffset;
  uint32_t rep0, rep1, rep2, rep3, state;
  // range coder
  uint64_t low, outPos;
  uint32_t range, cacheSize, cache;
  // driver
  uint32_t nowPos64, finished, overflow;

  // ---------------------------------------------------------------- range coder
  LZENC_FN void put_byte(uint32_t b) {
    if (outPos < dst_cap)
      dst[outPos] = uint8_t(b);
    else
      overflow = 1;
    ++outPos;
  }
  LZENC_FN void shift_low() {
    if (uint32_t(low) < 0xFF000000u || uint32_t(low >> 32) != 0) {
      uint32_t temp = cache;
      do {
        put_byte(temp + uint32_t(low >> 32));
        temp = 0xFF;
      } while (--cacheSize != 0);
      cache = uint32_t(low) >> 24;
    }
    cacheSize++;
    low = uint32_t(uint32_t(low) << 8);
  }
  LZENC_FN void flush_data() {
    for (int i = 0; i < 5; i++) shift_low();
  }
  LZENC_FN void encode_direct_bits(uint32_t value, int numBits) {
    do {
      range >>= 1;
      low += range & (0u - ((value >> --numBits) & 1));
      if (range < kTopValue) {
        range <<= 8;
        shift_low();
      }
    } while (numBits != 0);
  }
  LZENC_FN void encode_bit(uint32_t cell, uint32_t symbol) {
    uint32_t ttt = probs[cell];
    const uint32_t newBound = (range >> 11) * ttt;
    if (symbol == 0) {
      range = newBound;
      ttt += (2048 - ttt) >> 5;
    } else {
      low += newBound;
      range -= newBound;
      ttt -= ttt >> 5;
    }
    probs[cell] = uint16_t(ttt);
    if (range < kTopValue) {
      range <<= 8;
      shift_low();
    }
  }
  LZENC_FN void lit_encode(uint32_t base, uint32_t symbol) {
    symbol |= 0x100;
    do {
      encode_bit(base + (symbol >> 8), (symbol >> 7) & 1);
      symbol <<= 1;
    } while (symbol < 0x10000);
  }
  LZENC_FN void lit_encode_matched(uint32_t base, uint32_t symbol, uint32_t matchByte) {
    uint32_t offs = 0x100;
    symbol |= 0x100;
    do {
      matchByte <<= 1;
      encode_bit(base + offs + (matchByte & offs) + (symbol >> 8), (symbol >> 7) & 1);
      symbol <<= 1;
      offs &= ~(matchByte ^ symbol);
    } while (symbol < 0x10000);
  }
  LZENC_FN void tree_encode(uint32_t base, int numBitLevels, uint32_t symbol) {
    uint32_t m = 1;
    for (int i = numBitLevels; i != 0;) {
      i--;
      const uint32_t bit = (symbol >> i) & 1;
      encode_bit(base + m, bit);
      m = (m << 1) | bit;
    }
  }
  LZENC_FN void tree_reverse_encode(uint32_t base, int numBitLevels, uint32_t symbol) {
    uint32_t m = 1;
    for (int i = 0; i < numBitLevels; i++) {
      const uint32_t bit = symbol & 1;
      encode_bit(base + m, bit);
      m = (m << 1) | bit;
      symbol >>= 1;
    }
  }
  LZENC_FN void len_encode(uint32_t base, uint32_t symbol, uint32_t posState) {
    if (symbol < 8) {
      encode_bit(base, 0);
      tree_encode(base + kLenLow + (posState << 3), 3, symbol);
    } else {
      encode_bit(base, 1);
      if (symbol < 16) {
        encode_bit(base + 1, 0);
        tree_encode(base + kLenMid + (posState << 3), 3, symbol - 8);
      } else {
        encode_bit(base + 1, 1);
        tree_encode(base + kLenHigh, 8, symbol - 16);
      }
    }
  }

  // ---------------------------------------------------------------- prices (normal mode)
  // GET_PRICE, GET_PRICE_0, GET_PRICE_1 of a probability cell
  LZENC_FN uint32_t price_bit(uint32_t cell, uint32_t bit) const {
    return probPrices[(uint32_t(probs[cell]) ^ ((0u - bit) & 2047u)) >> 4];
  }
  LZENC_FN uint32_t price0(uint32_t cell) const { return probPrices[uint32_t(probs[cell]) >> 4]; }
  LZENC_FN uint32_t price1(uint32_t cell) const {
    return probPrices[(uint32_t(probs[cell]) ^ 2047u) >> 4];
  }
  LZENC_FN uint32_t lit_price(uint32_t base, uint32_t symbol) const {
    uint32_t price = 0;
    symbol |= 0x100;
    do {
      price += price_bit(base + (symbol >> 8), (symbol >> 7) & 1);
      symbol <<= 1;
    } while (symbol < 0x10000);
    return price;
  }
  LZENC_FN uint32_t lit_price_matched(uint32_t base, uint32_t symbol, uint32_t matchByte) const {
    uint32_t price = 0, offs = 0x100;
    symbol |= 0x100;
    do {
      matchByte <<= 1;
      price += price_bit(base + offs + (matchByte & offs) + (symbol >> 8), (symbol >> 7) & 1);
      symbol <<= 1;
      offs &= ~(matchByte ^ symbol);
    } while (symbol < 0x10000);
    return price;
  }
  LZENC_FN uint32_t tree_price(uint32_t base, int numBitLevels, uint32_t symbol) const {
    uint32_t price = 0;
    symbol |= 1u << numBitLevels;
    while (symbol != 1) {
      price += price_bit(base + (symbol >> 1), symbol & 1);
      symbol >>= 1;
    }
    return price;
  }
  LZENC_FN uint32_t tree_reverse_price(uint32_t base, int numBitLevels, uint32_t symbol) const {
    uint32_t price = 0, m = 1;
    for (int i = numBitLevels; i != 0; i--) {
      const uint32_t bit = symbol & 1;
      symbol >>= 1;
      price += price_bit(base + m, bit);
      m = (m << 1) | bit;
    }
    return price;
  }
  LZENC_FN uint32_t lit_probs(uint32_t pos, uint32_t prevByte) const {
    return kLit + (((pos & lpMask) << lc) + (prevByte >> (8 - lc))) * 0x300;
  }
  // which: 0 = lenEnc (cells at kLenEnc), 1 = repLenEnc (kRepLenEnc)
  LZENC_FN uint32_t* len_prices(uint32_t which, uint32_t posState) const {
    return lenPrices + ((which << pbBits) + posState) * kLenSymbols;
  }
  // LenPriceEnc_UpdateTable: LenEnc_SetPrices over tableSize symbols, then the counter
  LZENC_FN void len_update_table(uint32_t which, uint32_t posState) {
    const uint32_t base = which ? kRepLenEnc : kLenEnc;
    uint32_t* prices = len_prices(which, posState);
    const uint32_t a0 = price0(base), a1 = price1(base);
    const uint32_t b0 = a1 + price0(base + 1), b1 = a1 + price1(base + 1);
    const uint32_t numSymbols = lenTableSize;
    uint32_t i = 0;
    for (; i < 8 && i < numSymbols; i++)
      prices[i] = a0 + tree_price(base + kLenLow + (posState << 3), 3, i);
    for (; i < 16 && i < numSymbols; i++)
      prices[i] = b0 + tree_price(base + kLenMid + (posState << 3), 3, i - 8);
    for (; i < numSymbols; i++) prices[i] = b1 + tree_price(base + kLenHigh, 8, i - 16);
    prFixed[kPrLenCounters + which * 16 + posState] = lenTableSize;
  }
  // LenEnc_Encode2 with updatePrice
  LZENC_FN void len_encode2(uint32_t which, uint32_t symbol, uint32_t posState) {
    len_encode(which ? kRepLenEnc : kLenEnc, symbol, posState);
    if constexpr (kNormal) {
      if (!fastMode) {
        uint32_t* counter = prFixed + kPrLenCounters + which * 16 + posState;
        if (--*counter == 0) len_update_table(which, posState);
      }
    }
  }
  LZENC_FN void fill_align_prices() {
    for (uint32_t i = 0; i < kAlignTableSize; i++)
      prFixed[kPrAlign + i] = tree_reverse_price(kPosAlign, kNumAlignBits, i);
    alignPriceCount = 0;
  }
  LZENC_FN void fill_distances_prices() {
    uint32_t* tempPrices = prFixed + kPrTemp;
    for (uint32_t i = kStartPosModelIndex; i < kNumFullDistances; i++) {
      const uint32_t posSlot = get_pos_slot(i);
      const uint32_t footerBits = (posSlot >> 1) - 1;
      const uint32_t base = (2 | (posSlot & 1)) << footerBits;
      tempPrices[i] = tree_reverse_price(kPosEncoders + base - posSlot - 1, int(footerBits), i - base);
    }
    for (uint32_t lenToPosState = 0; lenToPosState < 4; lenToPosState++) {
      const uint32_t encoder = kPosSlot + lenToPosState * 64;
      uint32_t* posSlotPrices = prFixed + kPrPosSlot + lenToPosState * 64;
      for (uint32_t posSlot = 0; posSlot < distTableSize; posSlot++) {
        uint32_t price = tree_price(encoder, 6, posSlot);
        if (posSlot >= kEndPosModelIndex) price += (((posSlot >> 1) - 1) - kNumAlignBits) << 4;
        posSlotPrices[posSlot] = price;
      }
      // slots at or above distTableSize: the reference reads entries of
      // posSlotPrices it never wrote (zero in a fresh allocation).  Only
      // dictSize == 1 (distTableSize == 0, distance 0) ever uses such a price.
      uint32_t* distancesPrices = prFixed + kPrDistances + lenToPosState * kNumFullDistances;
      uint32_t i = 0;
      for (; i < kStartPosModelIndex; i++)
        distancesPrices[i] = i < distTableSize ? posSlotPrices[i] : 0u;
      for (; i < kNumFullDistances; i++) {
        const uint32_t slot = get_pos_slot(i);
        distancesPrices[i] = (slot < distTableSize ? posSlotPrices[slot] : 0u) + tempPrices[i];
      }
    }
    matchPriceCount = 0;
  }
  // LzmaEnc_InitPrices
  LZENC_FN void init_prices() {
    if (!fastMode) {
      fill_distances_prices();
      fill_align_prices();
      for (uint32_t posState = 0; posState < (1u << pbBits); posState++) len_update_table(0, posState);
      for (uint32_t posState = 0; posState < (1u << pbBits); posState++) len_update_table(1, posState);
    }
  }
  // price of distance `dist` after a match of length `len` (the two branches of
  // LzmaEnc.c:1087-1094)
  LZENC_FN uint32_t dist_price(uint32_t dist, uint32_t lenToPosState, uint32_t posSlot) const {
    if (dist < kNumFullDistances) return prFixed[kPrDistances + lenToPosState * kNumFullDistances + dist];
    return prFixed[kPrPosSlot + lenToPosState * 64 + posSlot] + prFixed[kPrAlign + (dist & 15)];
  }

  // ---------------------------------------------------------------- match finder
  LZENC_FN uint32_t avail() const { return src_len - off; }
  LZENC_FN void move_pos() {
    if (++cyclicBufferPos == cyclicBufferSize) cyclicBufferPos = 0;
    ++off;
  }
  // HASH4_CALC and the three table updates; returns the head of the 4-byte chain
  LZENC_FN uint32_t hash_insert(const uint8_t* cur, uint32_t pos, uint32_t* d2, uint32_t* d3) {
    const uint32_t temp = crc[cur[0]] ^ cur[1];
    const uint32_t hash2Value = temp & (kHash2Size - 1);
    const uint32_t hash3Value = (temp ^ (uint32_t(cur[2]) << 8)) & (kHash3Size - 1);
    const uint32_t hashValue = (temp ^ (uint32_t(cur[2]) << 8) ^ (crc[cur[3]] << 5)) & hashMask;
    *d2 = pos - hash[hash2Value];
    *d3 = pos - hash[kFix3HashSize + hash3Value];
    const uint32_t curMatch = hash[kFix4HashSize + hashValue];
    hash[hash2Value] = pos;
    hash[kFix3HashSize + hash3Value] = pos;
    hash[kFix4HashSize + hashValue] = pos;
    return curMatch;
  }
  LZENC_FN uint32_t hc_get_matches_spec(uint32_t lenLimit, uint32_t curMatch, uint32_t pos,
                                        const uint8_t* cur, uint32_t cutValue_, uint32_t offset,
                                        uint32_t maxLen) {
    son[cyclicBufferPos] = curMatch;
    for (;;) {
      const uint32_t delta = pos - curMatch;
      if (cutValue_-- == 0 || delta >= cyclicBufferSize || delta > off) return offset;
      const uint8_t* pb = cur - delta;
      curMatch = son[cyclicBufferPos - delta + ((delta > cyclicBufferPos) ? cyclicBufferSize : 0)];
      if (pb[maxLen] == cur[maxLen] && *pb == *cur) {
        uint32_t len = 0;
        while (++len != lenLimit)
          if (pb[len] != cur[len]) break;
        if (maxLen < len) {
          matches[offset++] = maxLen = len;
          matches[offset++] = delta - 1;
          if (len == lenLimit) return offset;
        }
      }
    }
  }
  // GetMatchesSpec1 (LzFind.c:353-406): `son` holds two words per ring slot,
  // the roots of the subtrees of smaller and of larger suffixes
  LZENC_FN uint32_t bt_get_matches_spec(uint32_t lenLimit, uint32_t curMatch, uint32_t pos,
                                        const uint8_t* cur, uint32_t cutValue_, uint32_t offset,
                                        uint32_t maxLen) {
    uint32_t ptr0 = (cyclicBufferPos << 1) + 1, ptr1 = cyclicBufferPos << 1;
    uint32_t len0 = 0, len1 = 0;
    for (;;) {
      const uint32_t delta = pos - curMatch;
      if (cutValue_-- == 0 || delta >= cyclicBufferSize || delta > off) {
        son[ptr0] = son[ptr1] = 0;
        return offset;
      }
      const uint32_t pair =
          (cyclicBufferPos - delta + ((delta > cyclicBufferPos) ? cyclicBufferSize : 0)) << 1;
      const uint8_t* pb = cur - delta;
      uint32_t len = len0 < len1 ? len0 : len1;
      if (pb[len] == cur[len]) {
        if (++len != lenLimit && pb[len] == cur[len])
          while (++len != lenLimit)
            if (pb[len] != cur[len]) break;
        if (maxLen < len) {
          matches[offset++] = maxLen = len;
          matches[offset++] = delta - 1;
          if (len == lenLimit) {
            son[ptr1] = son[pair];
            son[ptr0] = son[pair + 1];
            return offset;
          }
        }
      }
      if (pb[len] < cur[len]) {
        son[ptr1] = curMatch;
        ptr1 = pair + 1;
        curMatch = son[ptr1];
        len1 = len;
      } else {
        son[ptr0] = curMatch;
        ptr0 = pair;
        curMatch = son[ptr0];
        len0 = len;
      }
    }
  }
  // SkipMatchesSpec (LzFind.c:408-456)
  LZENC_FN void bt_skip_matches_spec(uint32_t lenLimit, uint32_t curMatch, uint32_t pos,
                                     const uint8_t* cur, uint32_t cutValue_) {
    uint32_t ptr0 = (cyclicBufferPos << 1) + 1, ptr1 = cyclicBufferPos << 1;
    uint32_t len0 = 0, len1 = 0;
    for (;;) {
      const uint32_t delta = pos - curMatch;
      if (cutValue_-- == 0 || delta >= cyclicBufferSize || delta > off) {
        son[ptr0] = son[ptr1] = 0;
        return;
      }
      const uint32_t pair =
          (cyclicBufferPos - delta + ((delta > cyclicBufferPos) ? cyclicBufferSize : 0)) << 1;
      const uint8_t* pb = cur - delta;
      uint32_t len = len0 < len1 ? len0 : len1;
      if (pb[len] == cur[len]) {
        while (++len != lenLimit)
          if (pb[len] != cur[len]) break;
        if (len == lenLimit) {
          son[ptr1] = son[pair];
          son[ptr0] = son[pair + 1];
          return;
        }
      }
      if (pb[len] < cur[len]) {
        son[ptr1] = curMatch;
        ptr1 = pair + 1;
        curMatch = son[ptr1];
        len1 = len;
      } else {
        son[ptr0] = curMatch;
        ptr0 = pair;
        curMatch = son[ptr0];
        len0 = len;
      }
    }
  }
  // Bt4_MatchFinder_GetMatches (LzFind.c:539-584)
  LZENC_FN uint32_t bt_get_matches() {
    uint32_t lenLimit = avail();
    if (lenLimit > numFastBytes) lenLimit = numFastBytes;
    if (lenLimit < 4) {
      move_pos();
      return 0;
    }
    const uint8_t* cur = src + off;
    const uint32_t pos = cyclicBufferSize + off;
    uint32_t delta2, delta3;
    const uint32_t curMatch = hash_insert(cur, pos, &delta2, &delta3);
    uint32_t maxLen = 1, offset = 0;
    if (delta2 < cyclicBufferSize && delta2 <= off && *(cur - delta2) == *cur) {
      matches[0] = maxLen = 2;
      matches[1] = delta2 - 1;
      offset = 2;
    }
    if (delta2 != delta3 && delta3 < cyclicBufferSize && delta3 <= off && *(cur - delta3) == *cur) {
      maxLen = 3;
      matches[offset + 1] = delta3 - 1;
      offset += 2;
      delta2 = delta3;
    }
    if (offset != 0) {
      for (; maxLen != lenLimit; maxLen++)
        if (*(cur + maxLen - delta2) != cur[maxLen]) break;
      matches[offset - 2] = maxLen;
      if (maxLen == lenLimit) {
        bt_skip_matches_spec(lenLimit, curMatch, pos, cur, cutValue);
        move_pos();
        return offset;
      }
    }
    if (maxLen < 3) maxLen = 3;
    offset = bt_get_matches_spec(lenLimit, curMatch, pos, cur, cutValue, offset, maxLen);
    move_pos();
    return offset;
  }
  // Bt4_MatchFinder_Skip (LzFind.c:688-702)
  LZENC_FN void bt_skip(uint32_t num) {
    do {
      uint32_t lenLimit = avail();
      if (lenLimit > numFastBytes) lenLimit = numFastBytes;
      if (lenLimit < 4) {
        move_pos();
        continue;
      }
      uint32_t delta2, delta3;
      const uint8_t* cur = src + off;
      const uint32_t pos = cyclicBufferSize + off;
      const uint32_t curMatch = hash_insert(cur, pos, &delta2, &delta3);
      bt_skip_matches_spec(lenLimit, curMatch, pos, cur, cutValue);
      move_pos();
    } while (--num != 0);
  }
  // Hc4_MatchFinder_GetMatches into `matches`; returns 2 * pairs
  LZENC_FN uint32_t get_matches() {
    if constexpr (kNormal) {
      if (btMode) return bt_get_matches();
    }
    uint32_t lenLimit = avail();
    if (lenLimit > numFastBytes) lenLimit = numFastBytes;
    if (lenLimit < 4) {
      move_pos();
      return 0;
    }
    const uint8_t* cur = src + off;
    const uint32_t pos = cyclicBufferSize + off;
    uint32_t delta2, delta3;
    const uint32_t curMatch = hash_insert(cur, pos, &delta2, &delta3);
    uint32_t maxLen = 1, offset = 0;
    if (delta2 < cyclicBufferSize && delta2 <= off && *(cur - delta2) == *cur) {
      matches[0] = maxLen = 2;
      matches[1] = delta2 - 1;
      offset = 2;
    }
    if (delta2 != delta3 && delta3 < cyclicBufferSize && delta3 <= off && *(cur - delta3) == *cur) {
      maxLen = 3;
      matches[offset + 1] = delta3 - 1;
      offset += 2;
      delta2 = delta3;
    }
    if (offset != 0) {
      for (; maxLen != lenLimit; maxLen++)
        if (*(cur + maxLen - delta2) != cur[maxLen]) break;
      matches[offset - 2] = maxLen;
      if (maxLen == lenLimit) {
        son[cyclicBufferPos] = curMatch;
        move_pos();
        return offset;
      }
    }
    if (maxLen < 3) maxLen = 3;
    offset = hc_get_matches_spec(lenLimit, curMatch, pos, cur, cutValue, offset, maxLen);
    move_pos();
    return offset;
  }
  // Hc4_MatchFinder_Skip
  LZENC_FN void skip(uint32_t num) {
    if constexpr (kNormal) {
      if (btMode) {
        bt_skip(num);
        return;
      }
    }
    do {
      if (avail() < 4) {  // lenLimit < 4 (numFastBytes >= 5)
        move_pos();
        continue;
      }
      uint32_t delta2, delta3;
      const uint32_t curMatch = hash_insert(src + off, cyclicBufferSize + off, &delta2, &delta3);
      son[cyclicBufferPos] = curMatch;
      move_pos();
    } while (--num != 0);
  }

  // ---------------------------------------------------------------- parser
  LZENC_FN void parser_move_pos(uint32_t num) {
    if (num != 0) {
      additionalOffset += num;
      skip(num);
    }
  }
  LZENC_FN_RMD uint32_t read_match_distances(uint32_t* numDistancePairsRes) {
    uint32_t lenRes = 0;
    numAvail = avail();
    const uint32_t pairs = get_matches();
    if (pairs > 0) {
      lenRes = matches[pairs - 2];
      if (lenRes == numFastBytes) {
        const uint8_t* pby = src + off - 1;
        const uint32_t distance = matches[pairs - 1] + 1;
        uint32_t na = numAvail;
        if (na > kMatchLenMax) na = kMatchLenMax;
        const uint8_t* pby2 = pby - distance;
        for (; lenRes < na && pby[lenRes] == pby2[lenRes]; lenRes++) {
        }
      }
    }
    additionalOffset++;
    *numDistancePairsRes = pairs;
    return lenRes;
  }
  LZENC_FN uint32_t rep(uint32_t i) const {
    return i == 0 ? rep0 : i == 1 ? rep1 : i == 2 ? rep2 : rep3;
  }
  static LZENC_FN bool change_pair(uint32_t smallDist, uint32_t bigDist) {
    return (bigDist >> 7) > smallDist;
  }
  LZENC_FN uint32_t get_optimum_fast(uint32_t* backRes) {
    uint32_t mainLen, mainDist, pairs, repIndex, repLen;
    if (additionalOffset == 0)
      mainLen = read_match_distances(&pairs);
    else {
      mainLen = longestMatchLength;
      pairs = numPairs;
    }
    uint32_t na = numAvail;
    *backRes = 0xFFFFFFFFu;
    if (na < 2) return 1;
    if (na > kMatchLenMax) na = kMatchLenMax;
    const uint8_t* data = src + off - 1;

    repLen = repIndex = 0;
    for (uint32_t i = 0; i < kNumReps; i++) {
      const uint8_t* data2 = data - (rep(i) + 1);
      if (data[0] != data2[0] || data[1] != data2[1]) continue;
      uint32_t len;
      for (len = 2; len < na && data[len] == data2[len]; len++) {
      }
      if (len >= numFastBytes) {
        *backRes = i;
        parser_move_pos(len - 1);
        return len;
      }
      if (len > repLen) {
        repIndex = i;
        repLen = len;
      }
    }

    if (mainLen >= numFastBytes) {
      *backRes = matches[pairs - 1] + kNumReps;
      parser_move_pos(mainLen - 1);
      return mainLen;
    }

    mainDist = 0;
    if (mainLen >= 2) {
      mainDist = matches[pairs - 1];
      while (pairs > 2 && mainLen == matches[pairs - 4] + 1) {
        if (!change_pair(matches[pairs - 3], mainDist)) break;
        pairs -= 2;
        mainLen = matches[pairs - 2];
        mainDist = matches[pairs - 1];
      }
      if (mainLen == 2 && mainDist >= 0x80) mainLen = 1;
    }

    if (repLen >= 2 && ((repLen + 1 >= mainLen) || (repLen + 2 >= mainLen && mainDist >= (1u << 9)) ||
                        (repLen + 3 >= mainLen && mainDist >= (1u << 15)))) {
      *backRes = repIndex;
      parser_move_pos(repLen - 1);
      return repLen;
    }

    if (mainLen < 2 || na <= 2) return 1;

    longestMatchLength = read_match_distances(&numPairs);
    if (longestMatchLength >= 2) {
      const uint32_t newDistance = matches[numPairs - 1];
      if ((longestMatchLength >= mainLen && newDistance < mainDist) ||
          (longestMatchLength == mainLen + 1 && !change_pair(mainDist, newDistance)) ||
          (longestMatchLength > mainLen + 1) ||
          (longestMatchLength + 1 >= mainLen && mainLen >= 3 && change_pair(newDistance, mainDist)))
        return 1;
    }

    data = src + off - 1;
    for (uint32_t i = 0; i < kNumReps; i++) {
      const uint8_t* data2 = data - (rep(i) + 1);
      if (data[0] != data2[0] || data[1] != data2[1]) continue;
      const uint32_t limit = mainLen - 1;
      uint32_t len;
      for (len = 2; len < limit && data[len] == data2[len]; len++) {
      }
      if (len >= limit) return 1;
    }
    *backRes = mainDist + kNumReps;
    parser_move_pos(mainLen - 2);
    return mainLen;
  }

  // ---------------------------------------------------------------- optimal parser
  // GetRepLen1Price, GetPureRepPrice (LzmaEnc.c:856-883)
  LZENC_FN uint32_t rep_len1_price(uint32_t st, uint32_t posState) const {
    return price0(kIsRepG0 + st) + price0(kIsRep0Long + st * 16 + posState);
  }
  LZENC_FN uint32_t pure_rep_price(uint32_t repIndex, uint32_t st, uint32_t posState) const {
    if (repIndex == 0) return price0(kIsRepG0 + st) + price1(kIsRep0Long + st * 16 + posState);
    uint32_t price = price1(kIsRepG0 + st);
    if (repIndex == 1)
      price += price0(kIsRepG1 + st);
    else
      price += price1(kIsRepG1 + st) + price_bit(kIsRepG2 + st, repIndex - 2);
    return price;
  }
  static LZENC_FN uint32_t sel4(uint32_t i, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return i == 0 ? a : i == 1 ? b : i == 2 ? c : d;
  }
  // length of the match at distance rep + 1 (0 when shorter than 2), up to limit
  LZENC_FN uint32_t rep_match_len(const uint8_t* data, uint32_t rep_, uint32_t limit) const {
    const uint8_t* data2 = data - (rep_ + 1);
    if (data[0] != data2[0] || data[1] != data2[1]) return 0;
    uint32_t lenTest;
    for (lenTest = 2; lenTest < limit && data[lenTest] == data2[lenTest]; lenTest++) {
    }
    return lenTest;
  }
  // Backward (LzmaEnc.c:891-927)
  LZENC_FN uint32_t backward(uint32_t* backRes, uint32_t cur) {
    uint32_t posMem = opt[cur].posPrev;
    uint32_t backMem = opt[cur].backPrev;
    optimumEndIndex = cur;
    do {
      if (opt[cur].prev1IsChar) {
        opt[posMem].backPrev = 0xFFFFFFFFu;
        opt[posMem].prev1IsChar = 0;
        opt[posMem].posPrev = posMem - 1;
        if (opt[cur].prev2) {
          opt[posMem - 1].prev1IsChar = 0;
          opt[posMem - 1].posPrev = opt[cur].posPrev2;
          opt[posMem - 1].backPrev = opt[cur].backPrev2;
        }
      }
      const uint32_t posPrev = posMem;
      const uint32_t backCur = backMem;
      backMem = opt[posPrev].backPrev;
      posMem = opt[posPrev].posPrev;
      opt[posPrev].backPrev = backCur;
      opt[posPrev].posPrev = cur;
      cur = posPrev;
    } while (cur != 0);
    *backRes = opt[0].backPrev;
    optimumCurrentIndex = opt[0].posPrev;
    return optimumCurrentIndex;
  }
  // lenEnd raised to `to`, the new cells at kInfinityPrice
  LZENC_FN void extend_opt(uint32_t* lenEnd, uint32_t to) {
    while (*lenEnd < to) opt[++*lenEnd].price = kInfinityPrice;
  }
  // GetOptimum (LzmaEnc.c:929-1485).  reps[] and repLens[] are named scalars
  // picked by selects, so that no run-time index sends them to scratch.
  LZENC_FN uint32_t get_optimum(uint32_t position, uint32_t* backRes) {
    if (optimumEndIndex != optimumCurrentIndex) {
      const uint32_t posPrev = opt[optimumCurrentIndex].posPrev;
      const uint32_t lenRes = posPrev - optimumCurrentIndex;
      *backRes = opt[optimumCurrentIndex].backPrev;
      optimumCurrentIndex = posPrev;
      return lenRes;
    }
    optimumCurrentIndex = optimumEndIndex = 0;

    uint32_t mainLen, pairs;
    if (additionalOffset == 0)
      mainLen = read_match_distances(&pairs);
    else {
      mainLen = longestMatchLength;
      pairs = numPairs;
    }
    uint32_t na = numAvail;
    if (na < 2) {
      *backRes = 0xFFFFFFFFu;
      return 1;
    }
    if (na > kMatchLenMax) na = kMatchLenMax;

    const uint8_t* data = src + off - 1;
    uint32_t r0 = rep0, r1 = rep1, r2 = rep2, r3 = rep3;
    const uint32_t repLen0 = rep_match_len(data, r0, na), repLen1 = rep_match_len(data, r1, na),
                   repLen2 = rep_match_len(data, r2, na), repLen3 = rep_match_len(data, r3, na);
    uint32_t repMaxIndex = 0, repMaxLen = repLen0;
    if (repLen1 > repMaxLen) {
      repMaxIndex = 1;
      repMaxLen = repLen1;
    }
    if (repLen2 > repMaxLen) {
      repMaxIndex = 2;
      repMaxLen = repLen2;
    }
    if (repLen3 > repMaxLen) {
      repMaxIndex = 3;
      repMaxLen = repLen3;
    }
    if (repMaxLen >= numFastBytes) {
      *backRes = repMaxIndex;
      parser_move_pos(repMaxLen - 1);
      return repMaxLen;
    }
    if (mainLen >= numFastBytes) {
      *backRes = matches[pairs - 1] + kNumReps;
      parser_move_pos(mainLen - 1);
      return mainLen;
    }
    uint32_t curByte = *data;
    uint32_t matchByte = *(data - (r0 + 1));
    if (mainLen < 2 && curByte != matchByte && repMaxLen < 2) {
      *backRes = 0xFFFFFFFFu;
      return 1;
    }

    opt[0].state = state;
    uint32_t posState = position & pbMask;
    {
      const uint32_t lit = lit_probs(position, *(data - 1));
      opt[1].price = price0(kIsMatch + state * 16 + posState) +
                     (state >= 7 ? lit_price_matched(lit, curByte, matchByte) : lit_price(lit, curByte));
    }
    opt[1].backPrev = 0xFFFFFFFFu;
    opt[1].prev1IsChar = 0;

    uint32_t matchPrice = price1(kIsMatch + state * 16 + posState);
    uint32_t repMatchPrice = matchPrice + price1(kIsRep + state);
    if (matchByte == curByte) {
      const uint32_t shortRepPrice = repMatchPrice + rep_len1_price(state, posState);
      if (shortRepPrice < opt[1].price) {
        opt[1].price = shortRepPrice;
        opt[1].backPrev = 0;
        opt[1].prev1IsChar = 0;
      }
    }
    uint32_t lenEnd = mainLen >= repMaxLen ? mainLen : repMaxLen;
    if (lenEnd < 2) {
      *backRes = opt[1].backPrev;
      return 1;
    }

    opt[1].posPrev = 0;
    opt[0].backs[0] = r0;
    opt[0].backs[1] = r1;
    opt[0].backs[2] = r2;
    opt[0].backs[3] = r3;

    {
      uint32_t len = lenEnd;
      do opt[len--].price = kInfinityPrice;
      while (len >= 2);
    }

    for (uint32_t i = 0; i < kNumReps; i++) {
      uint32_t repLen = sel4(i, repLen0, repLen1, repLen2, repLen3);
      if (repLen < 2) continue;
      const uint32_t price = repMatchPrice + pure_rep_price(i, state, posState);
      const uint32_t* lp_ = len_prices(1, posState);
      do {
        const uint32_t curAndLenPrice = price + lp_[repLen - 2];
        if (curAndLenPrice < opt[repLen].price) {
          opt[repLen].price = curAndLenPrice;
          opt[repLen].posPrev = 0;
          opt[repLen].backPrev = i;
          opt[repLen].prev1IsChar = 0;
        }
      } while (--repLen >= 2);
    }

    {
      const uint32_t normalMatchPrice = matchPrice + price0(kIsRep + state);
      uint32_t len = repLen0 >= 2 ? repLen0 + 1 : 2;
      if (len <= mainLen) {
        const uint32_t* lp_ = len_prices(0, posState);
        uint32_t offs = 0;
        while (len > matches[offs]) offs += 2;
        for (;; len++) {
          const uint32_t distance = matches[offs + 1];
          const uint32_t curAndLenPrice =
              normalMatchPrice + lp_[len - kMatchLenMin] +
              dist_price(distance, len_to_pos_state(len), get_pos_slot(distance));
          if (curAndLenPrice < opt[len].price) {
            opt[len].price = curAndLenPrice;
            opt[len].posPrev = 0;
            opt[len].backPrev = distance + kNumReps;
            opt[len].prev1IsChar = 0;
          }
          if (len == matches[offs]) {
            offs += 2;
            if (offs == pairs) break;
          }
        }
      }
    }

    uint32_t cur = 0;
    for (;;) {
      cur++;
      if (cur == lenEnd) return backward(backRes, cur);

      uint32_t newPairs;
      uint32_t newLen = read_match_distances(&newPairs);
      if (newLen >= numFastBytes) {
        numPairs = newPairs;
        longestMatchLength = newLen;
        return backward(backRes, cur);
      }
      position++;
      uint32_t posPrev = opt[cur].posPrev;
      const uint32_t curPrev1IsChar = opt[cur].prev1IsChar;
      const uint32_t curPrev2 = curPrev1IsChar ? opt[cur].prev2 : 0u;
      uint32_t st;
      if (curPrev1IsChar) {
        posPrev--;
        if (curPrev2) {
          st = opt[opt[cur].posPrev2].state;
          st = opt[cur].backPrev2 < kNumReps ? rep_next(st) : match_next(st);
        } else
          st = opt[posPrev].state;
        st = lit_next(st);
      } else
        st = opt[posPrev].state;
      if (posPrev == cur - 1) {
        st = opt[cur].backPrev == 0 ? short_rep_next(st) : lit_next(st);
      } else {
        uint32_t pos;
        if (curPrev1IsChar && curPrev2) {
          posPrev = opt[cur].posPrev2;
          pos = opt[cur].backPrev2;
          st = rep_next(st);
        } else {
          pos = opt[cur].backPrev;
          st = pos < kNumReps ? rep_next(st) : match_next(st);
        }
        const uint32_t b0 = opt[posPrev].backs[0], b1 = opt[posPrev].backs[1],
                       b2 = opt[posPrev].backs[2];
        if (pos < kNumReps) {
          const uint32_t b3 = opt[posPrev].backs[3];
          r0 = sel4(pos, b0, b1, b2, b3);
          r1 = pos >= 1 ? b0 : b1;
          r2 = pos >= 2 ? b1 : b2;
          r3 = pos >= 3 ? b2 : b3;
        } else {
          r0 = pos - kNumReps;
          r1 = b0;
          r2 = b1;
          r3 = b2;
        }
      }
      opt[cur].state = st;
      opt[cur].backs[0] = r0;
      opt[cur].backs[1] = r1;
      opt[cur].backs[2] = r2;
      opt[cur].backs[3] = r3;

      const uint32_t curPrice = opt[cur].price;
      bool nextIsChar = false;
      data = src + off - 1;
      curByte = *data;
      matchByte = *(data - (r0 + 1));
      posState = position & pbMask;

      uint32_t curAnd1Price = curPrice + price0(kIsMatch + st * 16 + posState);
      {
        const uint32_t lit = lit_probs(position, *(data - 1));
        curAnd1Price +=
            st >= 7 ? lit_price_matched(lit, curByte, matchByte) : lit_price(lit, curByte);
      }
      const uint32_t next = cur + 1;
      if (curAnd1Price < opt[next].price) {
        opt[next].price = curAnd1Price;
        opt[next].posPrev = cur;
        opt[next].backPrev = 0xFFFFFFFFu;
        opt[next].prev1IsChar = 0;
        nextIsChar = true;
      }

      matchPrice = curPrice + price1(kIsMatch + st * 16 + posState);
      repMatchPrice = matchPrice + price1(kIsRep + st);

      if (matchByte == curByte && !(opt[next].posPrev < cur && opt[next].backPrev == 0)) {
        const uint32_t shortRepPrice = repMatchPrice + rep_len1_price(st, posState);
        if (shortRepPrice <= opt[next].price) {
          opt[next].price = shortRepPrice;
          opt[next].posPrev = cur;
          opt[next].backPrev = 0;
          opt[next].prev1IsChar = 0;
          nextIsChar = true;
        }
      }
      uint32_t numAvailFull = numAvail;
      {
        const uint32_t temp = kNumOpts - 1 - cur;
        if (temp < numAvailFull) numAvailFull = temp;
      }
      if (numAvailFull < 2) continue;
      na = numAvailFull <= numFastBytes ? numAvailFull : numFastBytes;

      if (!nextIsChar && matchByte != curByte) {
        // try Literal + rep0
        const uint8_t* data2 = data - (r0 + 1);
        uint32_t limit = numFastBytes + 1;
        if (limit > numAvailFull) limit = numAvailFull;
        uint32_t temp;
        for (temp = 1; temp < limit && data[temp] == data2[temp]; temp++) {
        }
        const uint32_t lenTest2 = temp - 1;
        if (lenTest2 >= 2) {
          const uint32_t state2 = lit_next(st);
          const uint32_t posStateNext = (position + 1) & pbMask;
          const uint32_t nextRepMatchPrice = curAnd1Price +
                                             price1(kIsMatch + state2 * 16 + posStateNext) +
                                             price1(kIsRep + state2);
          const uint32_t offset = cur + 1 + lenTest2;
          extend_opt(&lenEnd, offset);
          const uint32_t curAndLenPrice = nextRepMatchPrice +
                                          len_prices(1, posStateNext)[lenTest2 - kMatchLenMin] +
                                          pure_rep_price(0, state2, posStateNext);
          if (curAndLenPrice < opt[offset].price) {
            opt[offset].price = curAndLenPrice;
            opt[offset].posPrev = cur + 1;
            opt[offset].backPrev = 0;
            opt[offset].prev1IsChar = 1;
            opt[offset].prev2 = 0;
          }
        }
      }

      uint32_t startLen = 2;
      for (uint32_t repIndex = 0; repIndex < kNumReps; repIndex++) {
        const uint8_t* data2 = data - (sel4(repIndex, r0, r1, r2, r3) + 1);
        if (data[0] != data2[0] || data[1] != data2[1]) continue;
        uint32_t lenTest;
        for (lenTest = 2; lenTest < na && data[lenTest] == data2[lenTest]; lenTest++) {
        }
        extend_opt(&lenEnd, cur + lenTest);
        const uint32_t lenTestTemp = lenTest;
        const uint32_t price = repMatchPrice + pure_rep_price(repIndex, st, posState);
        const uint32_t* lp_ = len_prices(1, posState);
        do {
          const uint32_t curAndLenPrice = price + lp_[lenTest - 2];
          const uint32_t at = cur + lenTest;
          if (curAndLenPrice < opt[at].price) {
            opt[at].price = curAndLenPrice;
            opt[at].posPrev = cur;
            opt[at].backPrev = repIndex;
            opt[at].prev1IsChar = 0;
          }
        } while (--lenTest >= 2);
        lenTest = lenTestTemp;

        if (repIndex == 0) startLen = lenTest + 1;

        {
          uint32_t lenTest2 = lenTest + 1;
          uint32_t limit = lenTest2 + numFastBytes;
          if (limit > numAvailFull) limit = numAvailFull;
          for (; lenTest2 < limit && data[lenTest2] == data2[lenTest2]; lenTest2++) {
          }
          lenTest2 -= lenTest + 1;
          if (lenTest2 >= 2) {
            uint32_t state2 = rep_next(st);
            uint32_t posStateNext = (position + lenTest) & pbMask;
            const uint32_t curAndLenCharPrice =
                price + lp_[lenTest - 2] + price0(kIsMatch + state2 * 16 + posStateNext) +
                lit_price_matched(lit_probs(position + lenTest, data[lenTest - 1]), data[lenTest],
                                  data2[lenTest]);
            state2 = lit_next(state2);
            posStateNext = (position + lenTest + 1) & pbMask;
            const uint32_t nextRepMatchPrice = curAndLenCharPrice +
                                               price1(kIsMatch + state2 * 16 + posStateNext) +
                                               price1(kIsRep + state2);
            const uint32_t offset = cur + lenTest + 1 + lenTest2;
            extend_opt(&lenEnd, offset);
            const uint32_t curAndLenPrice = nextRepMatchPrice +
                                            len_prices(1, posStateNext)[lenTest2 - kMatchLenMin] +
                                            pure_rep_price(0, state2, posStateNext);
            if (curAndLenPrice < opt[offset].price) {
              opt[offset].price = curAndLenPrice;
              opt[offset].posPrev = cur + lenTest + 1;
              opt[offset].backPrev = 0;
              opt[offset].prev1IsChar = 1;
              opt[offset].prev2 = 1;
              opt[offset].posPrev2 = cur;
              opt[offset].backPrev2 = repIndex;
            }
          }
        }
      }

      if (newLen > na) {
        newLen = na;
        for (newPairs = 0; newLen > matches[newPairs]; newPairs += 2) {
        }
        matches[newPairs] = newLen;
        newPairs += 2;
      }
      if (newLen >= startLen) {
        const uint32_t normalMatchPrice = matchPrice + price0(kIsRep + st);
        extend_opt(&lenEnd, cur + newLen);
        const uint32_t* lp_ = len_prices(0, posState);
        uint32_t offs = 0;
        while (startLen > matches[offs]) offs += 2;
        uint32_t curBack = matches[offs + 1];
        uint32_t posSlot = get_pos_slot(curBack);
        for (uint32_t lenTest = startLen;; lenTest++) {
          const uint32_t curAndLenPrice = normalMatchPrice + lp_[lenTest - kMatchLenMin] +
                                          dist_price(curBack, len_to_pos_state(lenTest), posSlot);
          const uint32_t at = cur + lenTest;
          if (curAndLenPrice < opt[at].price) {
            opt[at].price = curAndLenPrice;
            opt[at].posPrev = cur;
            opt[at].backPrev = curBack + kNumReps;
            opt[at].prev1IsChar = 0;
          }
          if (lenTest == matches[offs]) {
            // try Match + Literal + Rep0
            const uint8_t* data2 = data - (curBack + 1);
            uint32_t lenTest2 = lenTest + 1;
            uint32_t limit = lenTest2 + numFastBytes;
            if (limit > numAvailFull) limit = numAvailFull;
            for (; lenTest2 < limit && data[lenTest2] == data2[lenTest2]; lenTest2++) {
            }
            lenTest2 -= lenTest + 1;
            if (lenTest2 >= 2) {
              uint32_t state2 = match_next(st);
              uint32_t posStateNext = (position + lenTest) & pbMask;
              const uint32_t curAndLenCharPrice =
                  curAndLenPrice + price0(kIsMatch + state2 * 16 + posStateNext) +
                  lit_price_matched(lit_probs(position + lenTest, data[lenTest - 1]),
                                    data[lenTest], data2[lenTest]);
              state2 = lit_next(state2);
              posStateNext = (posStateNext + 1) & pbMask;
              const uint32_t nextRepMatchPrice = curAndLenCharPrice +
                                                 price1(kIsMatch + state2 * 16 + posStateNext) +
                                                 price1(kIsRep + state2);
              const uint32_t offset = cur + lenTest + 1 + lenTest2;
              extend_opt(&lenEnd, offset);
              const uint32_t curAndLenPrice2 = nextRepMatchPrice +
                                               len_prices(1, posStateNext)[lenTest2 - kMatchLenMin] +
                                               pure_rep_price(0, state2, posStateNext);
              if (curAndLenPrice2 < opt[offset].price) {
                opt[offset].price = curAndLenPrice2;
                opt[offset].posPrev = cur + lenTest + 1;
                opt[offset].backPrev = 0;
                opt[offset].prev1IsChar = 1;
                opt[offset].prev2 = 1;
                opt[offset].posPrev2 = cur;
                opt[offset].backPrev2 = curBack + kNumReps;
              }
            }
            offs += 2;
            if (offs == newPairs) break;
            curBack = matches[offs + 1];
            if (curBack >= kNumFullDistances) posSlot = get_pos_slot(curBack);
          }
        }
      }
    }
  }

  // ---------------------------------------------------------------- coder
  // kLiteralNextStates, kMatchNextStates, kRepNextStates, kShortRepNextStates
  static LZENC_FN uint32_t lit_next(uint32_t s) { return s < 4 ? 0 : s < 10 ? s - 3 : s - 6; }
  static LZENC_FN uint32_t match_next(uint32_t s) { return s < 7 ? 7 : 10; }
  static LZENC_FN uint32_t rep_next(uint32_t s) { return s < 7 ? 8 : 11; }
  static LZENC_FN uint32_t short_rep_next(uint32_t s) { return s < 7 ? 9 : 11; }
  static LZENC_FN uint32_t len_to_pos_state(uint32_t len) { return len < 5 ? len - 2 : 3; }
  static LZENC_FN uint32_t get_pos_slot(uint32_t pos) {
    if (pos < 2) return pos;
    const uint32_t i = 31 - uint32_t(__builtin_clz(pos));
    return (i + i) + ((pos >> (i - 1)) & 1);
  }

  LZENC_FN void write_end_marker(uint32_t posState) {
    encode_bit(kIsMatch + state * 16 + posState, 1);
    encode_bit(kIsRep + state, 0);
    state = match_next(state);
    const uint32_t len = kMatchLenMin;
    len_encode2(0, len - kMatchLenMin, posState);
    tree_encode(kPosSlot + len_to_pos_state(len) * 64, 6, (1 << 6) - 1);
    encode_direct_bits(((1u << 30) - 1) >> kNumAlignBits, 30 - kNumAlignBits);
    tree_reverse_encode(kPosAlign, kNumAlignBits, (1 << kNumAlignBits) - 1);
  }
  // CheckErrors: true when the stream has failed (the only failure is a write
  // that did not fit, the reference's rc.res / SZ_ERROR_WRITE)
  LZENC_FN bool check_errors() {
    if (overflow) finished = 1;
    return overflow != 0;
  }
  LZENC_FN void flush(uint32_t nowPos) {
    finished = 1;
    if (writeEndMark) write_end_marker(nowPos & pbMask);
    flush_data();
  }

  // GetOptimumFast or GetOptimum, by fastMode (LzmaEnc.c:1769-1772)
  LZENC_FN uint32_t next_token(uint32_t nowPos32, uint32_t* backRes) {
    if constexpr (kNormal) {
      if (!fastMode) return get_optimum(nowPos32, backRes);
    }
    return get_optimum_fast(backRes);
  }
  // the refresh of LzmaEnc.c:1868-1874, at additionalOffset == 0 only
  LZENC_FN void refresh_prices() {
    if constexpr (kNormal) {
      if (!fastMode) {
        if (matchPriceCount >= (1u << 7)) fill_distances_prices();
        if (alignPriceCount >= kAlignTableSize) fill_align_prices();
      }
    }
  }

  // LzmaEnc_CodeOneBlock.  kLimits == false is (p, False, 0, 0): a progress
  // step every 32 KiB.  kLimits == true is LZMA2's (p, True, 1 << 16, 1 << 21):
  // the chunk limits in place of the step, always ending in Flush, and no
  // CheckErrors on entry (the caller has just reset the output).
  //
  // kHold == true is a session's call (session_call below): src_len is what has
  // been supplied so far, and unless `finish` is set a token starts only while
  // src_len - nowPos >= hold, so that every "bytes left" the finder and the
  // parser look at during the token is at its clamp.  The block then returns
  // with the state as it stands -- additionalOffset may be 1, a literal whose
  // successor's matches are already read -- and a later call goes on from
  // there.  The other instantiations are the text they were.
  LZENC_FN void code_one_block() { code_block<false>(); }
  template <bool kLimits, bool kHold = false>
  LZENC_FN void code_block(uint32_t finish = 1, uint32_t hold = 0) {
    if constexpr (!kLimits) {
      if (check_errors()) return;
    }
    uint32_t nowPos32 = nowPos64;
    const uint32_t startPos32 = nowPos32;
    if constexpr (kHold) {
      if (!finish && src_len - nowPos32 < hold) return;
    }

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

    bool more = avail() != 0;
    if constexpr (kHold) more = more || additionalOffset != 0;  // a token read ahead is pending
    if (more)
      for (;;) {
        if constexpr (kHold) {
          if (!finish && src_len - nowPos32 < hold) {
            nowPos64 += nowPos32 - startPos32;
            return;
          }
        }
        uint32_t pos;
        const uint32_t len = next_token(nowPos32, &pos);
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
              len_encode2(1, len - kMatchLenMin, posState);
              state = rep_next(state);
            }
          } else {
            encode_bit(kIsRep + state, 0);
            state = match_next(state);
            len_encode2(0, len - kMatchLenMin, posState);
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
                if constexpr (kNormal) alignPriceCount++;
              }
            }
            rep3 = rep2;
            rep2 = rep1;
            rep1 = rep0;
            rep0 = pos;
            if constexpr (kNormal) matchPriceCount++;
          }
        }
        additionalOffset -= len;
        nowPos32 += len;
        if (additionalOffset == 0) {
          refresh_prices();
          if (avail() == 0) break;
          const uint32_t processed = nowPos32 - startPos32;
          if constexpr (kLimits) {
            // RangeEnc_GetProcessed: the chunk's bytes written plus cacheSize
            if (processed + kNumOpts + 300 >= kChunkUnpackMax ||
                outPos + cacheSize + kNumOpts * 2 >= kChunkPackMax)
              break;
          } else if (processed >= (1u << 15)) {
            nowPos64 += nowPos32 - startPos32;
            check_errors();
            return;
          }
        }
      }
    nowPos64 += nowPos32 - startPos32;
    flush(nowPos32);
  }

  // the normal-mode members (distTableSize: LzmaEnc.c:2023-2026)
  LZENC_FN void setup_normal(const Params& q, uint8_t* slice, const Layout& l,
                             const uint32_t* probPrices_) {
    fastMode = q.algo ? 0u : 1u;
    btMode = q.bt;
    pbBits = q.pb;
    probPrices = probPrices_;
    lenPrices = reinterpret_cast<uint32_t*>(slice + l.prices);
    prFixed = lenPrices + (2u << q.pb) * kLenSymbols;
    opt = reinterpret_cast<Opt*>(slice + l.opt);
    lenTableSize = q.fb + 1 - kMatchLenMin;
    uint32_t i;
    for (i = 0; i < 31; i++)
      if (q.dict_size <= (1u << i)) break;
    distTableSize = i * 2;
    optimumEndIndex = optimumCurrentIndex = 0;
    alignPriceCount = matchPriceCount = 0;
  }

  // LzmaEnc_MemEncode after LzmaEnc_SetProps: q has passed check_params
  LZENC_FN Out encode(const uint8_t* src_, uint32_t src_len_, uint8_t* dst_, uint64_t dst_cap_,
                      const Params& q, uint8_t* slice, const Layout& l, const uint32_t* crc_,
                      const uint32_t* probPrices_ = nullptr) {
    src = src_;
    dst = dst_;
    probs = reinterpret_cast<uint16_t*>(slice + l.probs);
    matches = reinterpret_cast<uint32_t*>(slice + l.matches);
    hash = reinterpret_cast<uint32_t*>(slice + l.hash);
    son = reinterpret_cast<uint32_t*>(slice + l.son);
    crc = crc_;
    src_len = src_len_;
    dst_cap = dst_cap_;
    lc = q.lc;
    lpMask = (1u << q.lp) - 1;
    pbMask = (1u << q.pb) - 1;
    numFastBytes = q.fb;
    cutValue = q.mc;
    writeEndMark = q.write_end_mark;
    hashMask = hash_mask(q.dict_size);
    cyclicBufferSize = q.dict_size + 1;
    // MatchFinder_Init
    off = 0;
    cyclicBufferPos = 0;
    // LzmaEnc_Init
    state = 0;
    rep0 = rep1 = rep2 = rep3 = 0;
    low = 0;
    range = 0xFFFFFFFFu;
    cacheSize = 1;
    cache = 0;
    outPos = 0;
    additionalOffset = 0;
    longestMatchLength = numPairs = numAvail = 0;
    nowPos64 = 0;
    finished = 0;
    overflow = 0;
    if constexpr (kNormal) {
      setup_normal(q, slice, l, probPrices_);
      init_prices();  // LzmaEnc_InitPrices; the cells are at kProbInit already
    }
    // LzmaEnc_Encode2
    for (;;) {
      code_one_block();
      if (finished) break;
    }
    Out o;
    o.res = overflow ? kErrOutputEof : kOk;
    o.dest_len = overflow ? dst_cap : outPos;
    return o;
  }

  // One call of an encoder session (fast path only): encode()'s loop, resumed
  // from and saved to the record S (LzmaEncGpuSession, include/lzma_gpu.h; a
  // template parameter so that this header needs no other).  src[0, src_len) is
  // the stream so far; the bytes of the earlier calls are still there, at the
  // same offsets, though not necessarily at the same address.  The slice
  // (lzmaenc_layout(q, src_cap)) has been through lzmaenc_init_slice before
  // the first call that finds work and is untouched since.  `hold` is
  // kSessionHold everywhere but in the test that shortens it.
  //
  // Why the bytes do not depend on the piece sizes.  The one-shot encoder looks
  // at the bytes left in three places: lenLimit = min(fb, left) in the finder,
  // numAvail (clamped to kMatchLenMax where it is used, read_match_distances
  // and get_optimum_fast; compared with 2 there as well), and `left < 4` in the
  // skip.  A token that starts at p steps the finder at positions p .. p + 272
  // only: its own read at p (made during the token before when
  // additionalOffset == 1), one read ahead at p + 1, then a skip to the last
  // byte of a match of at most kMatchLenMax.  With src_len - p >= 2 *
  // kMatchLenMax at the token's start, `left` is at least 274 at every one of
  // them: lenLimit is fb, numAvail is above its clamp, the skip hashes.  So each
  // of the three values decides what the full length would; the token and the
  // finder's tables are the one-shot encoder's, by induction over the tokens.
  // The check is made before every token, also one whose matches were read
  // ahead (additionalOffset == 1): a run of literals with read-ahead never
  // returns to additionalOffset == 0, and would otherwise outrun the input.
  template <class S>
  LZENC_FN void session_call(S& s, const uint32_t* crc_, uint32_t hold) {
    static_assert(!kNormal, "sessions are fast-path only");
    if (s.finished) return;  // done or dead: nothing changes
    const Params q = session_params(s);
    const int32_t bad = session_check(s);
    if (bad != kOk) {
      s.res = bad;
      s.status = kSessionFinished;
      s.finished = 1;
      return;
    }
    if (!s.finish && s.src_len - s.in_pos < hold) {
      s.status = kSessionNeedsInput;
      return;
    }
    const Layout l = lzmaenc_layout(q, s.src_cap);
    uint8_t* slice = static_cast<uint8_t*>(s.ws);
    src = s.src;
    dst = s.dst;
    probs = reinterpret_cast<uint16_t*>(slice + l.probs);
    matches = reinterpret_cast<uint32_t*>(slice + l.matches);
    hash = reinterpret_cast<uint32_t*>(slice + l.hash);
    son = reinterpret_cast<uint32_t*>(slice + l.son);
    crc = crc_;
    src_len = uint32_t(s.src_len);
    dst_cap = s.dst_cap;
    lc = q.lc;
    lpMask = (1u << q.lp) - 1;
    pbMask = (1u << q.pb) - 1;
    numFastBytes = q.fb;
    cutValue = q.mc;
    writeEndMark = q.write_end_mark;
    hashMask = hash_mask(q.dict_size);
    cyclicBufferSize = q.dict_size + 1;
    if (s.needs_init) {  // MatchFinder_Init and LzmaEnc_Init, as in encode()
      off = cyclicBufferPos = 0;
      state = 0;
      rep0 = rep1 = rep2 = rep3 = 0;
      low = 0;
      range = 0xFFFFFFFFu;
      cacheSize = 1;
      cache = 0;
      outPos = 0;
      additionalOffset = 0;
      longestMatchLength = numPairs = numAvail = 0;
      nowPos64 = 0;
      overflow = 0;
    } else {
      off = s.off;
      cyclicBufferPos = s.cyclic_pos;
      state = s.state;
      rep0 = s.reps[0];
      rep1 = s.reps[1];
      rep2 = s.reps[2];
      rep3 = s.reps[3];
      low = s.low;
      range = s.range;
      cacheSize = s.cache_size;
      cache = s.cache;
      outPos = s.out_total;
      additionalOffset = s.additional_offset;
      longestMatchLength = s.longest_match_length;
      numPairs = s.num_pairs;
      numAvail = s.num_avail;
      nowPos64 = uint32_t(s.in_pos);
      overflow = s.overflow;
      // a record that is not one this function saved steers no access: what
      // indexes memory is checked against what it is derived from
      uint32_t maxRep = rep0 > rep1 ? rep0 : rep1;
      if (rep2 > maxRep) maxRep = rep2;
      if (rep3 > maxRep) maxRep = rep3;
      if (additionalOffset > 1 || off != nowPos64 + additionalOffset || off > src_len ||
          cyclicBufferPos != off % cyclicBufferSize || state >= kNumStates ||
          maxRep >= nowPos64 || numPairs > kMatchesWords || (numPairs & 1)) {
        s.res = kErrParam;
        s.status = kSessionFinished;
        s.finished = 1;
        return;
      }
    }
    finished = 0;
    const uint32_t finish = s.finish ? 1u : 0u;
    const uint32_t startPos = nowPos64;
    int32_t status = kSessionNeedsInput;
    for (;;) {
      code_block<false, true>(finish, hold);
      if (finished) break;
      if (!finish && src_len - nowPos64 < hold) break;
      if (s.in_budget != 0 && nowPos64 - startPos >= s.in_budget) {
        status = kSessionBudget;
        break;
      }
    }
    // a write that did not fit ends the session now; the one-shot encoder goes
    // on to its next CheckErrors, with nothing more reaching dst
    if (overflow) finished = 1;
    s.needs_init = 0;
    s.off = off;
    s.cyclic_pos = cyclicBufferPos;
    s.state = state;
    s.reps[0] = rep0;
    s.reps[1] = rep1;
    s.reps[2] = rep2;
    s.reps[3] = rep3;
    s.low = low;
    s.range = range;
    s.cache_size = cacheSize;
    s.cache = cache;
    s.out_total = outPos;
    s.additional_offset = additionalOffset;
    s.longest_match_length = longestMatchLength;
    s.num_pairs = numPairs;
    s.num_avail = numAvail;
    s.overflow = overflow;
    s.finished = finished;
    s.in_pos = nowPos64;
    s.out_pos = overflow ? dst_cap : outPos;
    s.res = overflow ? kErrOutputEof : kOk;
    s.status = finished ? kSessionFinished : status;
  }
};
using LzmaEnc = LzmaEncT<false>;
using LzmaEncNormal = LzmaEncT<true>;

// Cells [first, first + step, ...) of a slice's probability tables to
// kProbInit and its hash words to 0: lane `first` of `step` (the host build is
// lane 0 of 1; on the device the whole grid shares the work).
LZENC_FN void lzmaenc_init_slice(uint8_t* slice, const Layout& l, uint64_t first, uint64_t step) {
  uint16_t* probs = reinterpret_cast<uint16_t*>(slice + l.probs);
  for (uint64_t i = first; i < l.prob_cells; i += step) probs[i] = uint16_t(kProbInit);
  uint32_t* hash = reinterpret_cast<uint32_t*>(slice + l.hash);
  for (uint64_t i = first; i < l.hash_words; i += step) hash[i] = 0;
}

// A fresh session record over the caller's buffers (host side): q has passed
// params_from_props.  Every field is written; the encoder's own are zero until
// the first call with work resets them (needs_init).
template <class S>
LZENC_HD void session_bind(S* s, const Params& q, const uint8_t* src, uint64_t src_cap,
                           uint8_t* dst, uint64_t dst_cap, void* ws) {
  S z = S();
  z.src = src;
  z.dst = dst;
  z.ws = ws;
  z.src_cap = src_cap;
  z.dst_cap = dst_cap;
  z.dict_size = q.dict_size;
  z.lc = q.lc;
  z.lp = q.lp;
  z.pb = q.pb;
  z.fb = q.fb;
  z.mc = q.mc;
  z.write_end_mark = q.write_end_mark;
  z.status = kSessionNeedsInput;
  z.needs_init = 1;
  *s = z;
}

}  // namespace lzenc
