// lzma_device.h -- per-lane LZMA decoder for CDNA4 (gfx950).
//
// One independent LZMA stream per lane.  Every lane runs the complete
// LzmaDec_DecodeToDic contract (LzmaDec.c:719-838) on its own state, so the
// observable results {res, status, destLen, srcLen} -- which depend on the
// reference's call segmentation: bulk pass bounded at inSize-20, one-symbol
// tail passes behind a dry-run look-ahead, the dictionary-size split -- are
// reproduced exactly, including truncated and corrupt streams.
//
// Probability tables use a compact, pb-dependent layout (the reference's
// layout is not observable): IsMatch / IsRep0Long / LenLow / LenMid are sized
// by the posStates actually reachable (1 << pb) instead of always 16.  The
// table splits into
//   lo : everything except the two 256-entry LenHigh trees -- the hot part,
//        kept in LDS by the fast kernel (ProbLo = LDS pointer) or in global
//        memory by the generic kernels (ProbLo = global pointer);
//   hi : the LenHigh trees (lengths >= 18, rare), always in global memory.
// lc=0/lp=0/pb=0: lo = 1262 cells (2,524 B), so 16 streams share a 40 KiB
// LDS slab and four such workgroups fill a CU.
//
// Other per-lane memory: dic = the caller's output window, which IS the
// dictionary (LzmaDecode, LzmaDec.c:988-989) or a ring of dicBufSize bytes;
// input = the compressed bytes, read through a register window refilled with
// aligned 4-byte loads one word ahead so NORMALIZE does not wait on memory.
//
// Reference map: bit/tree/direct-bit primitives LzmaDec.c:8-45,323-344;
// symbol loop :131-426 (lz_run); pending flush :428-452; dictionary split
// :454-477 (lz_run_split); look-ahead :487-675 (lz_probe); driver :719-838
// (lz_decode_to_dic); LZMA2 chunk walker Lzma2Dec.c:98-289 (lzma2_device.h).
#pragma once

#include <stdint.h>

#include <type_traits>

// LZGPU_HOST_EMU: the test-only host build of the per-lane logic (tests/emu)
// lets the CPU test suite exercise exactly this code before it runs on the GPU
#include "device_shim.h"

namespace lzgpu {

enum : int { kOk = 0, kErrData = 1, kErrMem = 2, kErrUnsupported = 4, kErrParam = 5, kErrInputEof = 6 };
// internal (never returned to a caller): the fast tail of a one-shot decode
// met a symbol that needs input past the stream's end; decode it again exactly
constexpr int kRetryExact = 99;
#ifndef LZGPU_FAST_TAIL
#define LZGPU_FAST_TAIL 1  // 0: probe every symbol of the last 20 bytes (A/B)
#endif
enum : int { kStNone = 0, kStDoneMark = 1, kStNotDone = 2, kStMoreInput = 3, kStMaybeDone = 4 };
enum : int { kFinAny = 0, kFinEnd = 1 };

constexpr uint32_t kTop = 1u << 24;
constexpr uint32_t kProbOne = 2048u;
constexpr uint32_t kProbInit = 1024u;
constexpr uint32_t kLookahead = 20u;  // LZMA_REQUIRED_INPUT_MAX
constexpr uint32_t kLenDone = 274u;   // kMatchSpecLenStart
// direct bits decided several per step on the cooperative kernel (direct_coop;
// -DLZGPU_DIRECT_CHUNKS=0 restores the bit-serial loop for A/B)
#ifndef LZGPU_DIRECT_CHUNKS
#define LZGPU_DIRECT_CHUNKS 1
#endif
constexpr bool kDirectChunks = LZGPU_DIRECT_CHUNKS != 0;

// ------------------------------------------------------------------ compact layout

// The probability table is stored as sections (cells = 16-bit probabilities,
// P = 1 << pb reachable posStates instead of the reference's fixed 16):
enum : uint32_t {
  S_MATCH,   // IsMatch[12][P]
  S_REP0L,   // IsRep0Long[12][P]
  S_REP,     // IsRep[12] IsRepG0[12] IsRepG1[12] IsRepG2[12]
  S_LEN,     // Len: choice, choice2, low[P][8], mid[P][8]
  S_REPLEN,  // RepLen: same
  S_SLOT,    // PosSlot[4][64]
  S_SPEC,    // SpecPos[114]
  S_ALIGN,   // Align[16]
  S_LITP,    // literal trees, plain part: [ctx][0x100]
  S_LITM,    // literal trees, matched part: [ctx][0x200] (reference offsets 0x100..0x2FF)
  S_LENHI,   // LenHigh[256] | RepLenHigh[256]
  S_NSEC
};

__host__ __device__ __forceinline__ uint32_t sec_cells(uint32_t sec, uint32_t lc, uint32_t lp,
                                                       uint32_t pb) {
  switch (sec) {
    case S_MATCH: case S_REP0L: return 12u << pb;
    case S_REP: return 48u;
    case S_LEN: case S_REPLEN: return 2u + (16u << pb);
    case S_SLOT: return 256u;
    case S_SPEC: return 114u;
    case S_ALIGN: return 16u;
    case S_LITP: return 256u << (lc + lp);
    case S_LITM: return 512u << (lc + lp);
    default: return 512u;  // S_LENHI
  }
}

// Section placement: bit s of `lds_mask` set = section s lives in the lane's
// LDS slice, otherwise in its global workspace slice (mask 0: all global).
// Offsets are assigned in section order within each of the two tables.
struct Layout {
  uint32_t o[S_NSEC];
  uint32_t lds_cells, glb_cells;
};
__host__ __device__ __forceinline__ Layout make_layout(uint32_t lc, uint32_t lp, uint32_t pb,
                                                       uint32_t lds_mask) {
  Layout L;
  uint32_t a = 0, b = 0;
  // literal sections first: every literal tree starts 8-byte aligned in
  // either table
  for (uint32_t k = 0; k < S_NSEC; ++k) {
    const uint32_t sec = k < 2 ? S_LITP + k : (k - 2 < S_LITP ? k - 2 : k);
    const uint32_t n = sec_cells(sec, lc, lp, pb);
    if ((lds_mask >> sec) & 1u) {
      L.o[sec] = a;
      a += n;
    } else {
      L.o[sec] = b;
      b += n;
    }
  }
  L.lds_cells = a;
  L.glb_cells = b;
  return L;
}
// Bit 29 of a placement mask (kSessHybBit, the time-sliced lane kernel): the
// mask's sections live in LDS, packed as usual, and the others stay at their
// offsets in the session's whole all-global table -- a round stages only the
// LDS sections in and out of the spilled table.
constexpr uint32_t kSessHybBit = 0x20000000u;
__host__ __device__ __forceinline__ Layout make_layout_m(uint32_t lc, uint32_t lp, uint32_t pb,
                                                         uint32_t m) {
  Layout L = make_layout(lc, lp, pb, m);
  if (m & kSessHybBit) {
    const Layout F = make_layout(lc, lp, pb, 0u);
    for (uint32_t k = 0; k < S_NSEC; ++k)
      if (!((m >> k) & 1u)) L.o[k] = F.o[k];
    L.glb_cells = F.glb_cells;
  }
  return L;
}

// whole table (all sections): 56P + 950 + 0x300 << (lc+lp) cells
__host__ __device__ __forceinline__ uint32_t table_cells(uint32_t lc, uint32_t lp, uint32_t pb) {
  return (56u << pb) + 950u + (768u << (lc + lp));
}
// reference numProbs (LzmaDec.c:110): what LzmaDec_AllocateProbs allocates;
// table_cells() <= num_probs() for every pb <= 4 (equal at pb = 4).
__host__ __device__ inline uint32_t num_probs(uint32_t lc, uint32_t lp) {
  return 1846u + (768u << (lc + lp));
}

// Placement used by the fast kernel (build-time; A/B'd on MI355X):
// default = only the per-symbol tables in LDS -- IsMatch, IsRep/G0/G1/G2 and the
// plain literal tree (632 B per lc0/pb0 stream: 256 resident streams per CU,
// 16 lanes x 4 waves per SIMD); the match path's tables live in global memory
// (+31 % over keeping them in LDS at half the resident streams).
#ifndef LZGPU_LDS_MASK
#define LZGPU_LDS_MASK 0x105u
#endif
// Placement for the latency regime (few streams per CU, one per wave): LDS is
// not the limit there, the match path's round trips are -- everything but
// SpecPos, the matched-literal trees and LenHigh stays in LDS.
#ifndef LZGPU_LDS_MASK_LAT
#define LZGPU_LDS_MASK_LAT 0x1BFu
#endif
// The latency placement with the slot trees in the global rows: a merged
// latency class whose widest slice (lc + lp = 4 at pb = 4: 5,316 cells) would
// take 9 of a CU's 128 LDS blocks runs 16 workgroups per CU at 8 blocks
// instead of 14 (the planner picks it only where it raises residency).
constexpr uint32_t kLdsMaskLatSlotG = LZGPU_LDS_MASK_LAT & ~(1u << S_SLOT);

// Explicit address spaces: LDS (3) for the lo table of the fast kernel, global
// (1) for everything else.  Generic pointers would compile to flat_* memory
// instructions, which count against both vmcnt and lgkmcnt -- every LDS wait
// would then also drain the lane's outstanding global stores.
#ifdef LZGPU_HOST_EMU
typedef uint16_t lds_u16;
typedef uint8_t gbyte;
typedef uint16_t gu16;
typedef uint32_t gu32;
#else
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(1))) uint8_t gbyte;
typedef __attribute__((address_space(1))) uint16_t gu16;
typedef __attribute__((address_space(1))) uint32_t gu32;
#endif

// Lane-interleaved global tables (placement bit kIlvBit, throughput kernel):
// the global sections of the 32 lanes of a lane group are stored cell-major --
// cell i of lane l at column l of row i (row = kIlv cells) -- so that lanes
// reading the same cell (choice bits, tree tops, IsRep0Long of one state) hit
// one 64-byte span instead of one line each, and a wave's frequently used
// cells share a few lines that stay cached.  GS is the lane's view: a pointer
// to its column with cell arithmetic scaled by the row length.
constexpr uint32_t kIlvBit = 0x40000000u;
constexpr uint32_t kIlv = 32u;
// Not a placement: the throughput kernel's W = 4 instantiations pass it down
// so that mp_on (round 9) stays off in them -- they spill at 128 VGPRs, the
// batches held across decisions would add 50 to 90 bytes of scratch each, and
// no benchmark measures them.  kRowBits: the bits a placement test ignores.
constexpr uint32_t kMpOffBit = 0x10000000u;
constexpr uint32_t kRowBits = kIlvBit | kMpOffBit;
struct GS {
  gu16* p;
  __device__ __forceinline__ GS operator+(uint32_t k) const { return GS{p + kIlv * k}; }
  __device__ __forceinline__ gu16& operator[](uint32_t k) const { return p[kIlv * k]; }
  __device__ __forceinline__ gu16& operator*() const { return *p; }
};
constexpr uint32_t kIlvLaneCells = 1u;
// The LDS slices of a lane-interleaved throughput class the same way (round 4):
// cell i of lane l of a 32-lane group at i * 32 + l, so the lanes' reads of
// different cells (tree nodes of diverging paths) fall in different LDS banks
// -- bank = (16 i + l / 2) mod 64 -- instead of colliding at random between
// per-lane slices (config 3: 79 M bank-conflict cycles per launch with slices).
// Not in the host emulation.  -DLZGPU_LDS_ILV=0 (A/B only) keeps per-lane slices.
#ifndef LZGPU_LDS_ILV
#define LZGPU_LDS_ILV 1
#endif
struct LS {
  lds_u16* p;
  __device__ __forceinline__ LS operator+(uint32_t k) const { return LS{p + kIlv * k}; }
  __device__ __forceinline__ lds_u16& operator[](uint32_t k) const { return p[kIlv * k]; }
  __device__ __forceinline__ lds_u16& operator*() const { return *p; }
};

// Build-time knobs still in use (A/B runs):
//   LZGPU_LIT_BATCH    literals decoded per pass of the symbol loop before a
//                      lane's match path runs (1 = one symbol per pass)
//   LZGPU_PROF         profiling build: wave-uniform cycle stamps per region
//   LZGPU_MP           the throughput match path's load batches (mp_on, round
//                      9): 1 length front, 2 LenHigh in three batches, 4 the
//                      distance tail's early batch (0 = round 8's path)
// The code shapes measured and rejected in rounds 1-2 (branch-free NORMALIZE,
// tree child-pair prefetch, two-round-trip literal trees, unified plain /
// matched literals, literal write-combining, byte-wise and batched-tail copies,
// threshold / divergent batch exits, nontemporal input / output, pair-
// interleaved rows, ...) were removed in round 3; their A/B evidence stays in
// DESIGN.md §4 and profiles/.  So were round 3's own rejects: the throughput
// copy taking the next matched byte from its own loads, deferred probability
// stores in the throughput match path, wave-uniform (ballot) branches in the
// cooperative and one-lane kernels (profiles/r03_storeack/).  The kept shapes
// are unconditional: decision and
// update as selects in the shared form, the checkpoint reader in the bulk pass
// of the throughput and cooperative placements (the 16-byte per-byte-checked
// reader elsewhere), the matched byte prefetched at match end (throughput and
// cooperative kernels), global bit trees three levels per load batch, the
// length coder / SpecPos / Align in fewer round trips off the throughput
// placement, the matched literal's eight all-match cells in one batch, match
// copies with unaligned 8-byte accesses, the wave-uniform literal-batch exit.
#ifndef LZGPU_LIT_BATCH
#define LZGPU_LIT_BATCH 8
#endif
// The decision's instruction form (Rc::decide), a bit mask of the kernels
// that take form 1: 1 the one-stream kernel (config 2 +2.6 %, config 5 +1 %),
// 4 the other batch kernels with an LDS placement -- throughput and one-lane
// latency (config 3 +2.6 % once the literal tree walks by address; -0.4 %
// before), 2 the cooperative kernels (config 4 -4 %, then -0.5 %: not taken).
// Default 5.  Kernels with no LDS placement bits (the generic batch kernel, the
// one-lane session kernel on a caller's CLzmaDec table) and the time-sliced
// session rounds (kSessHybBit) keep form 0: form 1's
// 16-bit update is exact only on cells the kernel initialised itself (round 6,
// DESIGN.md §4).
#ifndef LZGPU_BIT_FORM
#define LZGPU_BIT_FORM 5
#endif
#ifndef LZGPU_BIT16
#define LZGPU_BIT16 1  // form 1's update in 16-bit arithmetic (Rc::decide_b)
#endif
#ifndef LZGPU_PROF
#define LZGPU_PROF 0
#endif
// LZGPU_PROF=3 (profiling build, never the default; round 6, VERDICT r05 items
// 3-4): global-memory wait attribution.  At each class of global access the
// wave waits for all of its outstanding vector-memory operations (vmcnt(0))
// and the cycles of that wait go to the class: the stores queued before the
// match path (W_DRAIN), then each class's own loads.  The waits are taken one
// after another instead of overlapping, so the split says which class holds
// the wave, not the exact share of the default build's time.
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
enum : uint32_t {
  W_DRAIN,   // stores still queued at the match path's entry (literal bytes, table updates)
  W_MLIT,    // matched-literal cells (global placements)
  W_REP,     // IsRep0Long / rep-choice cells in global memory
  W_LEN,     // length coder
  W_SLOT,    // distance slot tree
  W_SPEC,    // SpecPos reverse trees
  W_ALIGN,   // Align reverse tree
  W_LENHI,   // LenHigh trees (lengths >= 18)
  W_COPY,    // match copies and short reps (dictionary reads + their stores)
  W_MB,      // the matched byte at rep0, loaded at match end
  W_INPUT,   // input blocks (reader refills)
  W_PREV,    // the previous byte at a pass's start, the look-ahead probe
  // (round 8; counters 36 and 37 of LzmaGpu_ProfileRead)
  W_FETCH,   // GlobalReaderQ: from a block fetch's issue to the end of a forced
             // wait behind it -- the wait the default build's copy of the
             // loaded block takes in the same place
  W_WALK,    // the wait at the head of the plain literal walk
  W_N
};
__device__ __forceinline__ void lz_wait_into(uint64_t& acc) {
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  acc += __builtin_amdgcn_s_memtime() - t0;
}
#define LZ_WAIT(arr, k) lz_wait_into((arr)[k])
#define LZ_WCLS(rc, k) ((rc).wcls = (k))
#else
#define LZ_WAIT(arr, k) ((void)0)
#define LZ_WCLS(rc, k) ((void)0)
#endif

// LDS history window (round 4, placement bit kWinBit, the wave-cooperative
// kernels): the most recent decoded bytes are kept in LDS as well as in the
// dictionary, so a match copy (and the matched literal's byte) at a distance
// the window covers is read from LDS instead of global memory -- where, in the
// in-order vmcnt queue, every such load waited for the wave's earlier output
// stores.  The window is a write-through cache of the
// dictionary's last `av` bytes: slot = write counter & mask.  `av` never
// exceeds `lim` = min(window bytes, dicBufSize): a ring smaller than the window
// (a caller's own dic under LzmaDec_AllocateProbs) holds only its last
// dicBufSize bytes, and a match reaching further reads the ring slot the
// reference reads (ring_back), overwritten or not.  Every byte the
// decoder writes goes to both; reads it cannot serve fall back to the
// dictionary, which is always complete.
constexpr uint32_t kWinBit = 0x08000000u;
#ifdef LZGPU_HOST_EMU
typedef uint8_t lds_u8;
#else
typedef __attribute__((address_space(3))) uint8_t lds_u8;
#endif
struct LzWin {
  lds_u8* b;
  uint32_t mask;  // window bytes - 1 (a power of two)
  uint32_t t;     // bytes written through the window
  uint32_t av;    // of them, still held and served (the last av, <= lim)
  uint32_t fl;    // of them, not yet stored to the dictionary (deferred output)
  uint32_t lim;   // av's cap: min(mask + 1, dicBufSize)
};
__host__ __device__ __forceinline__ LzWin win_make(lds_u8* b, uint32_t bytes, uint64_t cap) {
  return LzWin{b, bytes - 1, 0, 0, 0, uint32_t(cap < bytes ? cap : bytes)};
}
__device__ __forceinline__ void win_put(LzWin& w, uint32_t v) {
  w.b[w.t & w.mask] = uint8_t(v);
  ++w.t;
  w.av += (w.av < w.lim) ? 1u : 0u;
}
// the window after n more bytes were written through it
__device__ __forceinline__ void win_adv(LzWin& w, uint32_t n) {
  w.t += n;
  w.av = (w.av + n > w.lim) ? w.lim : w.av + n;
}
template <uint32_t M>
__host__ __device__ constexpr bool win_on() {
  return (M & kWinBit) != 0u;
}
// Deferred output (round 4; cooperative kernels with a window): decoded bytes
// go to the window only and reach the dictionary in bursts of >= kDeferBytes,
// stored by all lanes of the wave at once (win_flush), and before the bulk pass
// returns.  The last `fl` bytes are then missing from the dictionary, but
// nothing reads them there: a read at distance <= fl <= av is served by the
// window.  One store instruction per 32 bytes instead of one per literal, and
// far loads stop queueing behind the literal stores (in-order vmcnt).
// -DLZGPU_WIN_DEFER=0 (A/B only) writes every byte through.
#ifndef LZGPU_WIN_DEFER
#define LZGPU_WIN_DEFER 1
#endif
constexpr uint32_t kDeferBytes = 64u;

// A zero the compiler must treat as per-lane (written by an instruction it
// cannot see through).  The wave-cooperative kernels add it to their stream's
// offsets: every lane of such a wave holds the same decoder state, and with the
// state in registers (LzTmp below) the compiler proves that and moves the whole
// serial decoder to the scalar unit -- measured slower there (config 4 3,060 ->
// 2,607 MB/s: the scalar build spills hundreds of scalar registers to vector
// lanes; profiles/r04_tmp/, the A/B switch retired in round 5), so the
// cooperative state stays in vector registers.
__device__ __forceinline__ uint32_t lz_vzero() {
#if defined(LZGPU_HOST_EMU)
  return 0;
#else
  uint32_t z;
  asm volatile("v_mov_b32 %0, 0" : "=v"(z));
  return z;
#endif
}

// The lookahead buffer (CLzmaDec.tempBuf, LzmaDec.h:68: kLookahead bytes) as
// three 64-bit words.  As a byte array indexed by a run-time position it would
// be a dynamically indexed private array inside the decoder state, and the
// compiler keeps a structure that an unknown index reaches into in scratch
// memory as a whole -- the range coder, positions and reps included -- with
// every value read back from it a per-lane load; as words it is registers
// (round 4: config 3 +1.9 %, config 2 +2.3 %; the byte-array A/B build was
// retired in round 5).
struct LzTmp {
  uint64_t w0, w1, w2;
  __device__ __forceinline__ uint32_t get(uint32_t i) const {
    const uint64_t w = i < 8u ? w0 : (i < 16u ? w1 : w2);
    return uint32_t(w >> (8u * (i & 7u))) & 0xFFu;
  }
  __device__ __forceinline__ void set(uint32_t i, uint32_t b) {
    const uint32_t sh = 8u * (i & 7u);
    const uint64_t m = ~(uint64_t(0xFFu) << sh), v = uint64_t(b & 0xFFu) << sh;
    w0 = i < 8u ? ((w0 & m) | v) : w0;
    w1 = (i >= 8u && i < 16u) ? ((w1 & m) | v) : w1;
    w2 = i >= 16u ? ((w2 & m) | v) : w2;
  }
};
// byte pointer over an LzTmp (the look-ahead probe of the tempBuf path)
struct LzTmpIter {
  LzTmp t;
  uint32_t i;
  __device__ __forceinline__ LzTmpIter operator+(uint64_t n) const { return {t, i + uint32_t(n)}; }
  __device__ __forceinline__ bool operator>=(const LzTmpIter& o) const { return i >= o.i; }
  __device__ __forceinline__ uint32_t operator*() const { return t.get(i); }
  __device__ __forceinline__ LzTmpIter operator++(int) {
    const LzTmpIter r = *this;
    ++i;
    return r;
  }
};

// Per-lane decoder state (CLzmaDec fields, LzmaDec.h:50-69).  lo = the LDS
// table (pointer type Lo: lds_u16*; or gu16* aliasing gl when everything is
// global), gl = the global table.
template <class Lo>
struct LzStateT {
  uint32_t lc, lp, pb, dict_size;
  Lo lo;
  gu16* gl;
  gbyte* dic;
  uint64_t cap;   // dicBufSize
  uint64_t pos;   // dicPos
  uint32_t range, code;
  uint32_t total;  // processedPos
  uint32_t full;   // checkDicSize
  uint32_t st;
  uint32_t rep0, rep1, rep2, rep3;
  uint32_t pending;  // remainLen
  uint32_t need_rc_init, need_state_init;
  uint32_t tmp_n;
  LzTmp tmp;
  LzWin win;  // kWinBit placements only
#if LZGPU_PROF
  // [0..4] cycles: literal batches, match decode, copies + tail, calls, refills;
  // [5..13] wave-level counts: batch iterations, active / matched-literal lanes
  // per iteration, iterations with both literal kinds, match-path entries and
  // their lanes, live lanes per iteration, literals, matches (lane-level)
  // [14..16]: IsMatch, literal, batch tail cycles per literal; [17] literal
  // batch iterations; [18] the input tail (look-ahead dry runs + one-symbol
  // passes, LzmaDec.c:487-675 / :766-812), [19] tail passes, [20] table init
  uint64_t prof[21];
#endif
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
  uint64_t wprof[W_N];  // wait attribution (cycles per class)
#endif
};

template <uint32_t M>
__host__ __device__ constexpr bool lds_ilv() {
#ifdef LZGPU_HOST_EMU
  return false;
#else
  return LZGPU_LDS_ILV != 0 && (M & kIlvBit) != 0u;
#endif
}

// Section accessor for placement mask M (compile-time): at<S>(i) is a pointer to
// cell i of section S in whichever table holds it.
template <uint32_t M, class Lo>
struct Tab {
  Lo lo;
  gu16* gl;
  Layout L;
  __device__ __forceinline__ Tab(const LzStateT<Lo>& s)
      : lo(s.lo), gl(s.gl), L(make_layout_m(s.lc, s.lp, s.pb, M)) {}
  // cell `off` of the global table (lane-interleaved under kIlvBit)
  __device__ __forceinline__ auto g(uint32_t off) const {
    if constexpr ((M & kIlvBit) != 0u)
      return GS{gl + kIlv * off};
    else
      return gl + off;
  }
  template <uint32_t S>
  __device__ __forceinline__ auto at(uint32_t i) const {
    if constexpr (((M >> S) & 1u) != 0u) {
      if constexpr (lds_ilv<M>())
        return LS{lo + kIlv * (L.o[S] + i)};
      else
        return lo + (L.o[S] + i);
    } else {
      return g(L.o[S] + i);
    }
  }
};

__device__ __forceinline__ uint64_t ring_back(uint64_t pos, uint32_t dist, uint64_t cap) {
  return pos - dist + (pos < dist ? cap : 0);
}

// LZGPU_SHADOW_OUT (attribution build, never the default): every output
// store is repeated LZGPU_SHADOW_OUT bytes further on (the caller's buffer
// extends that far), so the L2 -> memory write traffic the output causes shows
// as the increase of WRITE_SIZE over the default build (traffic).
#ifndef LZGPU_SHADOW_OUT
#define LZGPU_SHADOW_OUT 0
#endif

// one decoded literal byte to the window
__device__ __forceinline__ void lz_put(gbyte* p, uint32_t v) {
  *p = uint8_t(v);
#if LZGPU_SHADOW_OUT
  p[LZGPU_SHADOW_OUT] = uint8_t(v);
#endif
}

// ------------------------------------------------------------------ input readers

// always-valid, 16-byte aligned target for exhausted prefetches
#ifdef LZGPU_HOST_EMU
alignas(16) static uint32_t g_lz_zero_word[4] = {0, 0, 0, 0};
#else
__device__ __attribute__((aligned(16))) uint32_t g_lz_zero_word[4] = {0, 0, 0, 0};
#endif


// Same contract, 16-byte refills: `win` holds up to 8 bytes; `nxt` is the
// next 16-byte aligned block (its low half is taken when win empties, the high
// half 8 bytes later, and only then is the following block requested), so one
// load and one drain per 16 input bytes.
// (Round 6 measured keeping the prefetched block in the load's own registers
// with wave-uniform refills on the one-stream and cooperative kernels -- the
// EXEC-masked refill copies the block at once, which waits for the load: config
// 4 -3.5 %, config 5 -0.9 %, config 2 +-0; the extra branches cost more than the
// waits.  DESIGN.md §4, round 6.)
struct GlobalReader16 {
  const gu32* wp;  // next 16-byte block to prefetch (as words)
  uint32_t left;   // 16-byte blocks with a valid byte still to prefetch
  uint32_t nb;     // valid bytes in win
  uint32_t half;   // 0: nxt untouched, 1: nxt low half already taken
  uint64_t win;
  uint64_t nlo, nhi;
  uint32_t taken;  // bytes moved into win since init (consumed = taken - nb)

  __device__ __forceinline__ void fetch() {
    // unconditional load (no phi on the loaded registers)
    const gu32* a = left ? wp : (const gu32*)g_lz_zero_word;
#ifdef LZGPU_HOST_EMU
    nlo = uint64_t(a[0]) | (uint64_t(a[1]) << 32);
    nhi = uint64_t(a[2]) | (uint64_t(a[3]) << 32);
#else
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = *(const __attribute__((address_space(1))) u32x4*)a;
    nlo = uint64_t(v.x) | (uint64_t(v.y) << 32);
    nhi = uint64_t(v.z) | (uint64_t(v.w) << 32);
#endif
    wp += left ? 4 : 0;
    left -= left ? 1u : 0u;
  }
  __device__ __forceinline__ void init(const gbyte* p, uint64_t avail) {
    const uintptr_t a = (uintptr_t)p;
    const uintptr_t a0 = a & ~uintptr_t(15);
    const uint32_t skip = uint32_t(a & 15);
    const uint64_t blocks = avail ? (((a + avail + 15) & ~uintptr_t(15)) - a0) >> 4 : 0;
    wp = (const gu32*)a0;
    left = blocks > 0xFFFFFFF0ull ? 0xFFFFFFF0u : uint32_t(blocks);
    fetch();  // first block: nlo/nhi
    if (skip < 8) {
      win = nlo >> (8 * skip);
      nb = 8 - skip;
      half = 1;
    } else {
      win = nhi >> (8 * (skip - 8));
      nb = 16 - skip;
      fetch();
      half = 0;
    }
    if (!avail) nb = 0;
    taken = nb;
  }
  __device__ __forceinline__ uint32_t used() const { return taken - nb; }
  __device__ __forceinline__ uint32_t peek() const { return uint32_t(win) & 0xFFu; }
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
  uint64_t prof = 0;
#endif
  __device__ __forceinline__ void refill() {
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
#endif
    if (half == 0) {
      win = nlo;
      half = 1;
    } else {
      win = nhi;
      fetch();
      half = 0;
    }
    nb = 8;
    taken += 8;
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
#if LZGPU_PROF == 3
    __builtin_amdgcn_s_waitcnt(0x0F70);  // the refill's load (W_INPUT)
#endif
    prof += __builtin_amdgcn_s_memtime() - t0;
#endif
  }
  __device__ __forceinline__ void advance(bool n) {
    if (n) {
      win >>= 8;
      --nb;
      if (nb == 0) refill();
    }
  }
  __device__ __forceinline__ uint32_t next() {
    const uint32_t b = peek();
    win >>= 8;
    --nb;
    if (nb == 0) refill();
    return b;
  }
};

// Checkpoint reader: NORMALIZE takes its byte from `win` without a refill
// check (take_u), and the decoder tops the window up at checkpoints where a
// bounded number of decisions follows (topup: nb <= 4 -> nb += 4, so >= 5
// bytes for the next <= 5 decisions).  The window is fed a 4-byte word at a
// time from the current 16-byte block (blo:bhi, bw words left); the next block
// is already loaded (nlo:nhi) when the current one runs out, and only then is
// the one after requested.  Same contract as GlobalReader16 otherwise:
// used() = bytes consumed, never loads a block wholly outside [p, p+avail).
struct GlobalReaderQ {
#ifdef LZGPU_HOST_EMU
  struct u32x4 { uint32_t x, y, z, w; };
#else
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#endif
  const gu32* wp;  // next 16-byte block to prefetch (as words)
  uint32_t left;   // blocks with a valid byte still to prefetch
  uint32_t nb;     // valid bytes in win (0..8)
  uint32_t bw;     // words left in blo:bhi (1..4)
  uint64_t win;
  uint64_t blo, bhi;
  // the prefetched next block, kept in the load's own register tuple: a copy
  // to other registers would make the compiler wait for the load right away
  u32x4 nx;
  uint32_t taken;  // bytes moved into win since init (consumed = taken - nb)
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
  uint64_t prof = 0;  // (refills are not timed separately in this reader)
  uint64_t prof_fetch = 0;  // LZGPU_PROF=3: W_FETCH
#endif

  __device__ __forceinline__ void fetch() {
    const gu32* a = left ? wp : (const gu32*)g_lz_zero_word;
#ifdef LZGPU_HOST_EMU
    nx = u32x4{a[0], a[1], a[2], a[3]};
#else
    nx = *(const __attribute__((address_space(1))) u32x4*)a;
#endif
    wp += left ? 4 : 0;
    left -= left ? 1u : 0u;
  }
  // drop the block's lowest word
  __device__ __forceinline__ void pop_word() {
    blo = (blo >> 32) | (bhi << 32);
    bhi >>= 32;
    if (--bw == 0) {
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
      lz_wait_into(prof);  // the prefetched block (wait attribution: W_INPUT)
#endif
      blo = uint64_t(nx.x) | (uint64_t(nx.y) << 32);
      bhi = uint64_t(nx.z) | (uint64_t(nx.w) << 32);
      bw = 4;
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
      const uint64_t t0 = __builtin_amdgcn_s_memtime();
      fetch();
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      prof_fetch += __builtin_amdgcn_s_memtime() - t0;
#else
      fetch();
#endif
    }
  }
  __device__ __forceinline__ void init(const gbyte* p, uint64_t avail) {
    const uintptr_t a = (uintptr_t)p;
    const uintptr_t a0 = a & ~uintptr_t(15);
    const uint64_t blocks = avail ? (((a + avail + 15) & ~uintptr_t(15)) - a0) >> 4 : 0;
    wp = (const gu32*)a0;
    left = blocks > 0xFFFFFFF0ull ? 0xFFFFFFF0u : uint32_t(blocks);
    fetch();
    blo = uint64_t(nx.x) | (uint64_t(nx.y) << 32);
    bhi = uint64_t(nx.z) | (uint64_t(nx.w) << 32);
    bw = 4;
    fetch();
    // skip the words of the first block before p, then the bytes of p's word
    for (uint32_t w = uint32_t(a & 15) >> 2; w != 0; --w) pop_word();
    const uint32_t sk = uint32_t(a & 3);
    win = uint64_t(uint32_t(blo)) >> (8 * sk);
    nb = avail ? 4 - sk : 0;
    pop_word();
    taken = nb;
  }
  __device__ __forceinline__ uint32_t used() const { return taken - nb; }
  __device__ __forceinline__ void topup() {
    if (nb <= 4) {
      win |= uint64_t(uint32_t(blo)) << (8 * nb);
      nb += 4;
      taken += 4;
      pop_word();
    }
  }
  __device__ __forceinline__ uint32_t peek() const { return uint32_t(win) & 0xFFu; }
  // next byte, no refill check (a checkpoint guaranteed nb > 0)
  __device__ __forceinline__ uint32_t take_u() {
    const uint32_t b = uint32_t(win) & 0xFFu;
    win >>= 8;
    --nb;
    return b;
  }
  __device__ __forceinline__ uint32_t next() {
    if (nb == 0) topup();
    return take_u();
  }
  __device__ __forceinline__ void advance(bool n) {
    if (n) {
      win >>= 8;
      --nb;
      if (nb == 0) topup();
    }
  }
};
// a value the compiler must not relate to the others (keeps a select of two
// registers a select)
template <class T>
__host__ __device__ __forceinline__ void lz_opaque(T& x) {
#ifndef LZGPU_HOST_EMU
  asm("" : "+v"(x));
#else
  (void)x;
#endif
}
// Input reader of the throughput placement (round 8):
//   0: GlobalReaderQ, as in the cooperative kernels; 1: GlobalReaderP
#ifndef LZGPU_READER
#define LZGPU_READER 1
#endif
// (a, b) = (x, y) as two register moves the compiler cannot fold into a use
// of x and y themselves, and a point no memory access is moved across: x and y
// are dead below it (host emulation: plain assignments)
__host__ __device__ __forceinline__ void lz_move2(uint64_t& a, uint64_t& b, uint64_t x,
                                                  uint64_t y) {
#ifndef LZGPU_HOST_EMU
  asm volatile("v_mov_b64 %0, %2\n\tv_mov_b64 %1, %3"
               : "=&v"(a), "=&v"(b)
               : "v"(x), "v"(y)
               : "memory");
#else
  a = x;
  b = y;
#endif
}
// GlobalReaderQ's contract with a prefetch that stays in flight.  In the
// throughput kernel GlobalReaderQ's fetch() is scheduled above the last read
// of the block it replaces, so the load gets a tuple of its own, is waited for
// at once (vmcnt(0): behind every store in flight too) and copied to nx -- a
// synchronous round trip on the decision chain at every block.  Here the
// promoted block's words are pinned in blo:bhi before the next fetch is issued
// (lz_move2), so the load lands in nx's own registers and the first wait that
// covers it is the promotion 16 input bytes later.
struct GlobalReaderP {
#ifdef LZGPU_HOST_EMU
  struct u32x4 { uint32_t x, y, z, w; };
#else
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#endif
  const gu32* wp;  // next 16-byte block to prefetch (as words)
  uint32_t left;   // blocks with a valid byte still to prefetch
  uint32_t nb;     // valid bytes in win (0..8)
  uint32_t bw;     // words left in blo:bhi (1..4)
  uint64_t win;
  uint64_t blo, bhi;
  u32x4 nx;        // the block in flight, in the load's own registers
  uint32_t taken;  // bytes moved into win since init (consumed = taken - nb)
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
  uint64_t prof = 0;        // LZGPU_PROF=3: the waits at promotions (W_INPUT)
  uint64_t prof_fetch = 0;  // (no wait behind a fetch in this reader)
#endif

  __device__ __forceinline__ void fetch() {
    const gu32* a = left ? wp : (const gu32*)g_lz_zero_word;
#ifdef LZGPU_HOST_EMU
    nx = u32x4{a[0], a[1], a[2], a[3]};
#else
    nx = *(const __attribute__((address_space(1))) u32x4*)a;
#endif
    wp += left ? 4 : 0;
    left -= left ? 1u : 0u;
  }
  // the prefetched block becomes the current one, then the next is requested
  __device__ __forceinline__ void promote() {
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
    lz_wait_into(prof);
#endif
    // nx's last read is here, the load below: nothing of nx is live across it
    lz_move2(blo, bhi, uint64_t(nx.x) | (uint64_t(nx.y) << 32),
             uint64_t(nx.z) | (uint64_t(nx.w) << 32));
    bw = 4;
    fetch();
  }
  __device__ __forceinline__ void pop_word() {
    blo = (blo >> 32) | (bhi << 32);
    bhi >>= 32;
    if (--bw == 0) promote();
  }
  // The checkpoint between the halves of a literal's tree walk: a promotion
  // there leaves its fetch to fetch_pending(), which the literal calls behind
  // the walk, before any other use of the reader.  The walk exists in two code
  // regions (plain, fused); a load issued inside them gives nx one definition
  // per region, and the copies that merge them at the join wait for the load.
  static constexpr uint32_t kFetchDue = 0x100u;
  __device__ __forceinline__ void topup_mid() {
    if (nb <= 4) {
      win |= uint64_t(uint32_t(blo)) << (8 * nb);
      nb += 4;
      taken += 4;
      blo = (blo >> 32) | (bhi << 32);
      bhi >>= 32;
      if (--bw == 0) {
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
        lz_wait_into(prof);
#endif
        blo = uint64_t(nx.x) | (uint64_t(nx.y) << 32);
        bhi = uint64_t(nx.z) | (uint64_t(nx.w) << 32);
        bw = 4 | kFetchDue;
      }
    }
  }
  __device__ __forceinline__ void fetch_pending() {
    if (bw > 4) {
      bw = 4;
      fetch();  // (nx's last read was topup_mid()'s)
    }
  }
  __device__ __forceinline__ void init(const gbyte* p, uint64_t avail) {
    const uintptr_t a = (uintptr_t)p;
    const uintptr_t a0 = a & ~uintptr_t(15);
    const uint64_t blocks = avail ? (((a + avail + 15) & ~uintptr_t(15)) - a0) >> 4 : 0;
    wp = (const gu32*)a0;
    left = blocks > 0xFFFFFFF0ull ? 0xFFFFFFF0u : uint32_t(blocks);
    fetch();
    promote();
    // skip the words of the first block before p, then the bytes of p's word
    for (uint32_t w = uint32_t(a & 15) >> 2; w != 0; --w) pop_word();
    const uint32_t sk = uint32_t(a & 3);
    win = uint64_t(uint32_t(blo)) >> (8 * sk);
    nb = avail ? 4 - sk : 0;
    pop_word();
    taken = nb;
  }
  __device__ __forceinline__ uint32_t used() const { return taken - nb; }
  __device__ __forceinline__ void topup() {
    if (nb <= 4) {
      win |= uint64_t(uint32_t(blo)) << (8 * nb);
      nb += 4;
      taken += 4;
      pop_word();
    }
  }
  __device__ __forceinline__ uint32_t peek() const { return uint32_t(win) & 0xFFu; }
  __device__ __forceinline__ uint32_t take_u() {
    const uint32_t b = uint32_t(win) & 0xFFu;
    win >>= 8;
    --nb;
    return b;
  }
  __device__ __forceinline__ uint32_t next() {
    if (nb == 0) topup();
    return take_u();
  }
  __device__ __forceinline__ void advance(bool n) {
    if (n) {
      win >>= 8;
      --nb;
      if (nb == 0) topup();
    }
  }
};
// the checkpoint readers (topup / take_u)
template <class Rd>
constexpr bool kIsQ = __is_same(Rd, GlobalReaderQ) || __is_same(Rd, GlobalReaderP);

typedef GlobalReader16 PlainReader;
// Reader of the bulk pass per placement: the checkpoint reader for the
// throughput placement (many lanes per wave: a refill check in every
// NORMALIZE fires in some lane almost every decision), the per-byte-checked
// one elsewhere (one lane per wave: config 2 5.8 vs 5.2 GB/s).
// Bit 31 of a placement mask marks the wave-cooperative kernel (kCoopBit: one
// stream per wave, every lane holding the same state).
constexpr uint32_t kCoopBit = 0x80000000u;
// Bit 26 of a placement mask marks the one-stream 32-lane kernel
// (lzgpu_decode_dup_kernel): every lane of the wave holds the same decoder
// state, as in the cooperative kernels, but the loads, stores and copies stay
// those of one lane.
constexpr uint32_t kDupBit = 0x04000000u;
template <uint32_t M>
__host__ __device__ constexpr bool bit_form() {
  constexpr uint32_t k = (M & kDupBit) != 0u    ? 1u
                         : (M & kCoopBit) != 0u ? 2u
                         : ((M & 0x7FFu) != 0u && (M & kSessHybBit) == 0u) ? 4u
                                                                           : 0u;
  return (LZGPU_BIT_FORM & k) != 0u;
}
// Plain literal tree walked by the cell's LDS address instead of the node
// (Rc::tree8_a): a' = 2a + (bit ? step - base : -base) is one select and one
// shift-add per level where the node form takes a shift, a 0 / 1 select, an
// or and the address's shift-add (and form 1 its bit-mask xor) -- config 2
// +1.9 %, config 3 +1.8 %, config 5 +0.6 %, config 4 +0.3 % (round 6,
// DESIGN.md §4).  Bit mask of kernels: 1 one-stream, 2 cooperative, 4 the
// others (throughput, one-lane latency); 7 = every kernel with the tree in LDS
// (default).  The same walk in the match path's LDS trees (length, slot,
// align) measured config 4 -1.3 %, config 2 -1 %, config 5 +0.9 % against it
// and was removed.
#ifndef LZGPU_LIT_ADDR
#define LZGPU_LIT_ADDR 7
#endif
template <uint32_t M>
__host__ __device__ constexpr bool lit_addr_on() {
  constexpr uint32_t k = (M & kDupBit) != 0u ? 1u : (M & kCoopBit) != 0u ? 2u : 4u;
  return ((M >> S_LITP) & 1u) != 0u && (LZGPU_LIT_ADDR & k) != 0u;
}
// Fused tree walks (round 7): lanes of a wave that need the same
// kind of walk over different cells take it in ONE code region on a per-lane
// base, instead of one EXEC-masked region per case after the other -- the wave
// pays every region's whole decision chain, whatever number of lanes use it.
// A fusion moves where a lane's decision is issued, never which decisions the
// lane makes or their order.  One bit per fusion:
//   1 (F1) length coder: LenLow and LenMid are one sub3 on a per-lane base
//   2 (F2) distance tail: SpecPos and Align are one reverse-tree walk with a
//          per-lane (base, bit count), behind the direct bits
//   8 (F4) literal: in an iteration where some lane decodes a matched literal,
//          all literal lanes take one 8-level walk (matched lanes from their
//          preloaded matched cells until the first mismatch)
// (4, F3, the rep chain by level, was not built; LenHigh's top three levels in
// F1's walk measured +0.8 %, inside three times the A/B spread, and were
// removed: DESIGN.md §4 round 7.)  Compiled only into the
// throughput placement, both row layouts: every other kernel's lanes either
// agree (one-stream, cooperative, sessions), where a per-lane select is pure
// cost, or were not measured (generic batch kernel, latency placement).
#ifndef LZGPU_FUSE
#define LZGPU_FUSE 11
#endif
template <uint32_t M>
__host__ __device__ constexpr bool fuse_on(uint32_t bit) {
  return (LZGPU_FUSE & bit) != 0u && (M & ~kRowBits) == LZGPU_LDS_MASK;
}
// The match path's dependent global round trips (round 9): a
// wave's entry walks choice -> choice2 -> length tree -> slot tree (two
// batches) -> distance tail, every step a load batch whose address needs the
// step before, each behind the earlier decisions' stores in the in-order
// vmcnt queue.  With lane-interleaved rows the cells that lanes share sit in
// one 64-byte row, so loading more cells per batch costs few extra lines.
// One bit per form; a load moves ahead of decisions that cannot store to its
// cells, never the decisions, their order, the input bytes or the updates:
//   1 length front: choice, choice2 and the low and mid trees of the lane's
//     posState in ONE batch on the per-lane coder base (Len or RepLen), issued
//     when IsRep is decided, ahead of the rep-distance bits (LDS), and decided
//     from registers (F1's one walk for low and mid kept)
//   2 LenHigh in three batches (tree8_g: 3 + 3 + 2 levels) instead of eight
//     dependent cells
//   4 distance tail: the reverse tree's first batch (seven cells on the
//     per-lane base, SpecPos + sp or Align) issued before the direct bits and
//     decided behind them; the last one or two levels from one batch
// (8, the slot tree's top issued early, was not built: DESIGN.md §4 round 9.)
// (A fourth tail level from the early batch, Align as sub4, measured inside
// three times the A/B spread and was removed.)
// Gated like fuse_on: the throughput placement only, both row layouts, and
// off under kMpOffBit (the W = 4 instantiations).
#ifndef LZGPU_MP
#define LZGPU_MP 7
#endif
template <uint32_t M>
__host__ __device__ constexpr bool mp_on(uint32_t bit) {
  return (LZGPU_MP & bit) != 0u && (M & kMpOffBit) == 0u && (M & ~kRowBits) == LZGPU_LDS_MASK;
}
// Some active lane of the wave wants the fused walk.  The host emulation is
// one lane wide: there -DLZGPU_FUSE_EMU_ALL=1 (tests only) answers "yes" for
// every literal, so that lanes which only follow a neighbour into the walk --
// plain literals in it -- are emulated too.
#ifndef LZGPU_FUSE_EMU_ALL
#define LZGPU_FUSE_EMU_ALL 0
#endif
__device__ __forceinline__ bool lz_fuse_any(bool v) {
#ifdef LZGPU_HOST_EMU
  return v || LZGPU_FUSE_EMU_ALL != 0;
#else
  return __builtin_amdgcn_ballot_w64(v) != 0;
#endif
}
// LDS cell addresses as integers (32-bit on the device)
#ifdef LZGPU_HOST_EMU
typedef uintptr_t lds_addr_t;
#else
typedef uint32_t lds_addr_t;
#endif
__host__ __device__ __forceinline__ lds_addr_t lds_addr_of(lds_u16* p) {
  return lds_addr_t(uintptr_t(p));
}
__host__ __device__ __forceinline__ lds_addr_t lds_addr_of(LS p) { return lds_addr_of(p.p); }
template <class P>
__host__ __device__ __forceinline__ P lds_at(lds_addr_t a);
template <>
__host__ __device__ __forceinline__ lds_u16* lds_at<lds_u16*>(lds_addr_t a) {
  return (lds_u16*)uintptr_t(a);
}
template <>
__host__ __device__ __forceinline__ LS lds_at<LS>(lds_addr_t a) {
  return LS{(lds_u16*)uintptr_t(a)};
}
template <class P>
constexpr lds_addr_t kLdsStep = __is_same(P, LS) ? lds_addr_t(2u * kIlv) : lds_addr_t(2u);
template <uint32_t M>
__host__ __device__ constexpr bool def_on() {
  return LZGPU_WIN_DEFER != 0 && win_on<M>() && (M & kCoopBit) != 0u;
}
// every section in LDS (cooperative classes with few streams per CU)
#ifndef LZGPU_LDS_MASK_ALL
#define LZGPU_LDS_MASK_ALL 0x7FFu
#endif
// Windowed cooperative builds (kWinBit) take the per-byte reader: measured
// faster than the checkpoint reader once the window is there -- config 4 3,187
// vs 3,060 MB/s, xz 2,834 vs 2,642, config 1 2.71 vs 2.49 MB/s
// (profiles/r04_tmp/, r04_qserial/).  Every kernel decides the plain literal
// tree one level at a time: the lane speculation of rounds 2-3 (5 + 3 levels
// per stage on the cooperative kernel) measured slower on the round-4 build
// everywhere it ran -- 8 LZMA2 blocks per CU 5,146 vs 5,494 MB/s, the windowed
// config 4 3,100 vs 3,318 MB/s (profiles/r04_coop8/, r04_qserial/) -- and was
// removed in round 5 with the other rejected shapes.
template <uint32_t M>
struct BulkReaderFor {
  static constexpr uint32_t m = M & ~kRowBits;
  static constexpr bool q = m == LZGPU_LDS_MASK || m == (LZGPU_LDS_MASK_LAT | kCoopBit) ||
                            m == (LZGPU_LDS_MASK_ALL | kCoopBit);
  // the throughput placement's own reader (LZGPU_READER)
  static constexpr bool p = LZGPU_READER != 0 && m == LZGPU_LDS_MASK;
  typedef typename std::conditional<
      p, GlobalReaderP,
      typename std::conditional<q, GlobalReaderQ, PlainReader>::type>::type type;
};

// Matched-byte prefetch per placement: the byte at rep0 is loaded at match end in
// the throughput and cooperative kernels; the one-stream-per-wave latency
// kernel loads it when the literal needs it -- the register the prefetch holds
// across the next IsMatch decision costs it scratch spills at 4 waves per SIMD
// (config 2 5.86 -> 6.12 GB/s, config 5 4.90 -> 5.03 without; config 3 and 4
// within noise either way: profiles/r02_ilv/mbpf_latency_ab.log)
template <uint32_t M>
__host__ __device__ constexpr bool mb_pf_on() {
  return ((M & kCoopBit) != 0u) || ((M & ~kRowBits) == LZGPU_LDS_MASK);
}

// checkpoint hooks for readers without them: every NORMALIZE checks
template <class Rd>
__device__ __forceinline__ void rd_topup(Rd& rd) {
  if constexpr (kIsQ<Rd>) rd.topup();
}
// the literal's mid-walk checkpoint and the fetch it may leave behind
template <class Rd>
__device__ __forceinline__ void rd_topup_mid(Rd& rd) {
  if constexpr (__is_same(Rd, GlobalReaderP))
    rd.topup_mid();
  else
    rd_topup(rd);
}
template <class Rd>
__device__ __forceinline__ void rd_fetch_pending(Rd& rd) {
  if constexpr (__is_same(Rd, GlobalReaderP)) rd.fetch_pending();
}
template <class Rd>
__device__ __forceinline__ uint32_t rd_take_u(Rd& rd) {
  if constexpr (kIsQ<Rd>)
    return rd.take_u();
  else
    return rd.next();
}

// Reader over a lane-private byte array (the tempBuf path).
struct LocalReader {
  LzTmp t;
  uint32_t idx;
  __device__ __forceinline__ void init(const LzTmp& q) { t = q; idx = 0; }
  __device__ __forceinline__ uint32_t used() const { return idx; }
  __device__ __forceinline__ uint32_t peek() const { return t.get(idx); }
  __device__ __forceinline__ void advance(bool n) { idx += n ? 1u : 0u; }
  __device__ __forceinline__ uint32_t next() { return t.get(idx++); }
};

// ------------------------------------------------------------------ range decoder

// The cooperative kernels' lanes all hold the same decoder state, so the
// decoder's branch conditions are wave-uniform there.
template <uint32_t M>
__host__ __device__ constexpr bool uni_on() {
  return (M & kCoopBit) != 0u;
}
// A wave-uniform branch condition tested as a ballot: the compiler branches on
// the compare's mask (VCC) instead of saving, narrowing and restoring EXEC
// around the body.  Measured (profiles/r05_uni/): the cooperative kernel,
// one wave per SIMD, +2.2 % on config 4 and +2.5 % on the xz leg; the 32-lane
// one-stream kernel, four waves per SIMD and issue-bound, lost 3.5 % on
// config 2 (the compiler materialises the conditions and adds phi copies), so
// it keeps EXEC-masked branches.
#ifndef LZGPU_UNI_IF
#define LZGPU_UNI_IF 2  // 0: plain (EXEC-masked) branches everywhere; 1: NORMALIZE only (A/B)
#endif
// Uniform symbol loop (round 6): where every lane holds the same state, the
// symbol loop decodes one symbol per pass and tests the symbol kind (IsMatch)
// and its exit as wave-uniform branches.  The literal batch (LZGPU_LIT_BATCH)
// exists to keep the independent streams of a wave together; on a uniform
// decoder it only costs lane-mask bookkeeping: its flags (literal run on,
// match found, stop) are loop-carried lane masks, ~40 scalar mask instructions
// per literal in the ISA of the one-stream kernel.
//   0: batch loop everywhere; 1: uniform loop in the one-stream kernel;
//   2: ... and in the cooperative kernels.
#ifndef LZGPU_UNI_LOOP
#define LZGPU_UNI_LOOP 2
#endif
template <uint32_t M>
__host__ __device__ constexpr bool uloop_on() {
  return (LZGPU_UNI_LOOP >= 1 && (M & kDupBit) != 0u) ||
         (LZGPU_UNI_LOOP >= 2 && (M & kCoopBit) != 0u);
}
// a condition every lane of the wave agrees on, as a uniform branch
__device__ __forceinline__ bool lz_uni(bool c) {
#ifndef LZGPU_HOST_EMU
  return __builtin_amdgcn_ballot_w64(c) != 0;
#else
  return c;
#endif
}
template <bool U>
__device__ __forceinline__ bool lz_if(bool c) {
#ifndef LZGPU_HOST_EMU
  if constexpr (U && LZGPU_UNI_IF != 0) return __builtin_amdgcn_ballot_w64(c) != 0;
#endif
  return c;
}
// the same for the symbol loop's own branches (symbol kind, rep kind, length
// choice, distance slot class); LZGPU_UNI_IF=1 keeps them EXEC-masked
template <bool U>
__device__ __forceinline__ bool lz_br(bool c) {
#ifndef LZGPU_HOST_EMU
  if constexpr (U && LZGPU_UNI_IF >= 2) return __builtin_amdgcn_ballot_w64(c) != 0;
#endif
  return c;
}

// F: the decision's instruction form (Rc::decide; bit_form<M>())
template <class P>
constexpr bool kGlobP = __is_same(P, gu16*) || __is_same(P, GS);
template <class Rd, bool U = false, bool F = false>
struct Rc {
  uint32_t range, code;
  Rd* rd;
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
  uint64_t* wacc = nullptr;  // wait attribution: accumulators, current class
  uint32_t wcls = 0;
  __device__ __forceinline__ void wstamp() {
    if (wacc) lz_wait_into(wacc[wcls]);
  }
#else
  __device__ __forceinline__ void wstamp() {}
#endif
  // NORMALIZE (LzmaDec.c:17): shift in one input byte when range < 2^24
  __device__ __forceinline__ void norm() {
    if (lz_if<U>(range < kTop)) {
      range <<= 8;
      code = (code << 8) | rd->next();
    }
  }
  // NORMALIZE after a reader checkpoint: the byte is known to be in the window
  __device__ __forceinline__ void norm_u() {
    if (lz_if<U>(range < kTop)) {
      range <<= 8;
      code = (code << 8) | rd_take_u(*rd);
    }
  }
  // The decision and its probability update on a loaded value p (after
  // NORMALIZE), IF_BIT_0 / UPDATE_0 / UPDATE_1 of LzmaDec.c:8-16.
  // Form 0 (rounds 1-5): selects only -- b = (code >= bound), p -= (p - m) >> 5
  // (arithmetic) with m = 2017 for bit 0 and 0 for bit 1 (UPDATE_0:
  // p + ((2048 - p) >> 5) == p - ((p - 2017) >> 5); UPDATE_1: p - (p >> 5)).
  // Form 1 (round 6, LZGPU_BIT_FORM): the subtraction's borrow is the bit
  // (v_sub_co: code - bound and code < bound in one instruction, the compare
  // gone) and the update is one multiply-add, p' = (31 p + c) >> 5 with
  // c = 31 for bit 1 and 2048 for bit 0: p - floor(p / 32) = floor((31 p + 31)
  // / 32) and p + floor((2048 - p) / 32) = floor((31 p + 2048) / 32) for every
  // 0 <= p <= 2048 (checked for all p by tests/test_emu.py).
  template <class P>
  __device__ __forceinline__ bool decide_b(uint32_t p, P prob) {
    const uint32_t bound = (range >> 11) * p;
    if constexpr (F) {
    uint32_t t;
    const bool borrow = __builtin_sub_overflow(code, bound, &t);
    code = borrow ? code : t;
    range = borrow ? bound : range - bound;
#if LZGPU_BIT16
    // 16-bit arithmetic: 31 p + c <= 31 * 2017 + 2048 < 2^16 -- a cell the
    // decoder initialised (1024) stays within [31, 2017] under both updates,
    // and form 1 runs only where the kernel initialises the table itself (the
    // batch kernels, bit_form) -- and a 16-bit multiply-add reads only the
    // cell's low half (no mask of the loaded value: one VALU instruction per
    // decision, round 6)
    const uint16_t p16 = uint16_t(p);
    const uint16_t c16 = borrow ? uint16_t(2048) : uint16_t(31);
    *prob = uint16_t(uint16_t(p16 * uint16_t(31) + c16) >> 5);
#else
    *prob = uint16_t((p * 31u + (borrow ? 2048u : 31u)) >> 5);
#endif
    return !borrow;
    } else {
    const bool b = code >= bound;
    const int32_t m = b ? 0 : int32_t(kProbOne - 31);
    *prob = uint16_t(int32_t(p) - ((int32_t(p) - m) >> 5));
    range = b ? range - bound : bound;
    code = b ? code - bound : code;
    return b;
    }
  }
  // The decision's value part alone -- decide_b's arithmetic with the cell's
  // new value returned in pn instead of stored: the fused literal walk
  // (lz_literal, fuse_on) stores it to the cell of the lane's class.  Kept
  // beside decide_b instead of under it, so that the kernels without fused
  // walks compile exactly as before.
  __device__ __forceinline__ bool decide_v(uint32_t p, uint16_t& pn) {
    const uint32_t bound = (range >> 11) * p;
    if constexpr (F) {
      uint32_t t;
      const bool borrow = __builtin_sub_overflow(code, bound, &t);
      code = borrow ? code : t;
      range = borrow ? bound : range - bound;
#if LZGPU_BIT16
      const uint16_t p16 = uint16_t(p);
      const uint16_t c16 = borrow ? uint16_t(2048) : uint16_t(31);
      pn = uint16_t(uint16_t(p16 * uint16_t(31) + c16) >> 5);
#else
      pn = uint16_t((p * 31u + (borrow ? 2048u : 31u)) >> 5);
#endif
      return !borrow;
    } else {
      const bool b = code >= bound;
      const int32_t m = b ? 0 : int32_t(kProbOne - 31);
      pn = uint16_t(int32_t(p) - ((int32_t(p) - m) >> 5));
      range = b ? range - bound : bound;
      code = b ? code - bound : code;
      return b;
    }
  }
  template <class P>
  __device__ __forceinline__ uint32_t decide(uint32_t p, P prob) {
    return decide_b(p, prob) ? 1u : 0u;
  }
  // bit_u as a condition (a branch on it needs no 0 / 1 value: the uniform
  // loop's IsMatch)
  template <class P>
  __device__ __forceinline__ bool bit_ub(P prob) {
    const uint32_t p = *prob;
    if constexpr (kGlobP<P>) wstamp();
    norm_u();
    if constexpr (F) {
      // the bit as its own compare: a branch on a compare result needs no
      // 0 / 1 value and mask rebuilt from it (the borrow of form 1 is one;
      // config 2 +1.2 % with the two changes beside it, round 6)
      const bool b = code >= (range >> 11) * p;
      decide_b(p, prob);
      return b;
    } else {
      return decide_b(p, prob);
    }
  }
  // decision with norm_u
  template <class P>
  __device__ __forceinline__ uint32_t bit_u(P prob) {
    const uint32_t p = *prob;
    if constexpr (kGlobP<P>) wstamp();
    norm_u();
    return decide(p, prob);
  }
  // decision on a preloaded value p with norm_u
  template <class P>
  __device__ __forceinline__ uint32_t bit_vu(uint32_t p, P prob) {
    norm_u();
    return decide(p, prob);
  }
  // BITS levels of an MSB-first tree from node m (no refill checks: at most
  // 5 levels after a checkpoint); returns the node reached
  template <int BITS, class P>
  __device__ __forceinline__ uint32_t tree_u(P probs, uint32_t m) {
#pragma unroll
    for (int k = 0; k < BITS; ++k) m = (m << 1) | bit_u(probs + m);
    return m;
  }
  // The 8-level plain literal tree (as tree_u<4> + rd_topup + tree_u<4>)
  // walked by the LDS address of the current cell (lit_addr_on); returns the
  // node (256..511).
  template <class P>
  __device__ __forceinline__ uint32_t tree8_a(P probs) {
    constexpr lds_addr_t st = kLdsStep<P>;
    const lds_addr_t base = lds_addr_of(probs);
    lds_addr_t k0 = lds_addr_t(0) - base, k1 = st - base;
    lz_opaque(k1);
    lds_addr_t a = base + st;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k == 4) rd_topup_mid(*rd);
      const uint32_t b = bit_u(lds_at<P>(a));
      a = (a << 1) + (b ? k1 : k0);
    }
    return uint32_t((a - base) / st);
  }
  // one adaptive decision on *prob (any address space), IF_BIT_0/UPDATE_0/1
  template <class P>
  __device__ __forceinline__ uint32_t bit(P prob) {
    const uint32_t p = *prob;
    if constexpr (kGlobP<P>) wstamp();
    norm();
    return decide(p, prob);
  }
  // decision on an already-loaded probability value p, update stored to *prob
  template <class P>
  __device__ __forceinline__ uint32_t bit_v(uint32_t p, P prob) {
    norm();
    return decide(p, prob);
  }
  // MSB-first bit tree of BITS levels (TREE_DECODE); returns [0, 1 << BITS)
  template <int BITS, class P>
  __device__ __forceinline__ uint32_t tree(P probs) {
    uint32_t m = 1;
#pragma unroll
    for (int k = 0; k < BITS; ++k) m = (m << 1) | bit(probs + m);
    return m - (1u << BITS);
  }
  // Three levels of a bit tree below node `root` (cells root, 2root + {0,1},
  // 4root + {0..3}) with all seven probabilities loaded in one batch: one
  // memory round trip instead of three dependent ones when the tree lives in
  // global memory.  Returns the node 8 * root + (the three bits, MSB first).
  template <class P>
  __device__ __forceinline__ uint32_t sub3(P probs, uint32_t root) {
    const uint32_t r2 = root * 2, r4 = root * 4;
    const uint32_t c0 = probs[root], c10 = probs[r2], c11 = probs[r2 + 1];
    const uint32_t c20 = probs[r4], c21 = probs[r4 + 1], c22 = probs[r4 + 2],
                   c23 = probs[r4 + 3];
    if constexpr (kGlobP<P>) wstamp();
    const uint32_t b0 = bit_v(c0, probs + root);
    uint32_t m = r2 + b0;
    const uint32_t b1 = bit_v(b0 ? c11 : c10, probs + m);
    m = 2 * m + b1;
    const uint32_t p2 = b0 ? (b1 ? c23 : c22) : (b1 ? c21 : c20);
    const uint32_t b2 = bit_v(p2, probs + m);
    return 2 * m + b2;
  }
  // Two levels below `root` (cells root, 2root + {0,1}) from one load batch;
  // returns 4 * root + (the two bits, MSB first).
  template <class P>
  __device__ __forceinline__ uint32_t sub2(P probs, uint32_t root) {
    const uint32_t c0 = probs[root], c10 = probs[2 * root], c11 = probs[2 * root + 1];
    if constexpr (kGlobP<P>) wstamp();
    const uint32_t b0 = bit_v(c0, probs + root);
    const uint32_t m = 2 * root + b0;
    const uint32_t b1 = bit_v(b0 ? c11 : c10, probs + m);
    return 2 * m + b1;
  }
  // Four levels below `root` (15 cells) from one load batch; returns
  // 16 * root + (the four bits, MSB first).  The candidates of the levels
  // below are halved by each decided bit (independent selects), so a level's
  // probability is one select behind its parent's decision.
  template <class P>
  __device__ __forceinline__ uint32_t sub4(P probs, uint32_t root) {
    auto dec = [&](uint32_t p, P cell) { return bit_v(p, cell); };
    const uint32_t r2 = root * 2, r4 = root * 4, r8 = root * 8;
    const uint32_t c1 = probs[root];
    uint32_t c2[2], c4[4], c8[8];
#pragma unroll
    for (int k = 0; k < 2; ++k) c2[k] = probs[r2 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) c4[k] = probs[r4 + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) c8[k] = probs[r8 + k];
    if constexpr (kGlobP<P>) wstamp();
    const uint32_t b0 = dec(c1, probs + root);
    uint32_t m = r2 + b0;
    const uint32_t p1 = b0 ? c2[1] : c2[0];
    const uint32_t q0 = b0 ? c4[2] : c4[0], q1 = b0 ? c4[3] : c4[1];
    uint32_t e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = b0 ? c8[4 + k] : c8[k];
    const uint32_t b1 = dec(p1, probs + m);
    m = 2 * m + b1;
    const uint32_t p2 = b1 ? q1 : q0;
    const uint32_t f0 = b1 ? e[2] : e[0], f1 = b1 ? e[3] : e[1];
    const uint32_t b2 = dec(p2, probs + m);
    m = 2 * m + b2;
    const uint32_t b3 = dec(b2 ? f1 : f0, probs + m);
    return 2 * m + b3;
  }
  // Seven cells of a 3-level subtree under `root`, loaded as one batch ahead of
  // the decisions that need them (dec3).
  template <class P>
  __device__ __forceinline__ void load7(P probs, uint32_t root, uint32_t* c) {
    c[0] = probs[root];
    c[1] = probs[2 * root];
    c[2] = probs[2 * root + 1];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[3 + k] = probs[4 * root + k];
  }
  template <class P>
  __device__ __forceinline__ uint32_t dec3(P probs, uint32_t root, const uint32_t* c) {
    if constexpr (kGlobP<P>) wstamp();
    const uint32_t b0 = bit_v(c[0], probs + root);
    uint32_t m = 2 * root + b0;
    const uint32_t b1 = bit_v(b0 ? c[2] : c[1], probs + m);
    m = 2 * m + b1;
    const uint32_t p2 = b0 ? (b1 ? c[6] : c[5]) : (b1 ? c[4] : c[3]);
    const uint32_t b2 = bit_v(p2, probs + m);
    return 2 * m + b2;
  }
  // dec3 on seven values (c1: the root's cell, c2 / c3 its children, c4..c7
  // theirs) instead of an array: where the batch is loaded well ahead of its
  // decisions (mp_on), dec3's choice between array cells kept the array in
  // scratch memory (32 bytes per site in the throughput builds).
  template <class P>
  __device__ __forceinline__ uint32_t dec3_v(P probs, uint32_t root, uint32_t c1, uint32_t c2,
                                             uint32_t c3, uint32_t c4, uint32_t c5, uint32_t c6,
                                             uint32_t c7) {
    if constexpr (kGlobP<P>) wstamp();
    const uint32_t b0 = bit_v(c1, probs + root);
    uint32_t m = 2 * root + b0;
    const uint32_t b1 = bit_v(b0 ? c3 : c2, probs + m);
    m = 2 * m + b1;
    const uint32_t p2 = b0 ? (b1 ? c7 : c6) : (b1 ? c5 : c4);
    const uint32_t b2 = bit_v(p2, probs + m);
    return 2 * m + b2;
  }
  // 8-level tree in global memory in three load batches (3 + 3 + 2 levels)
  // instead of eight dependent round trips; returns the node (256..511).
  template <class P>
  __device__ __forceinline__ uint32_t tree8_g(P probs) {
    return sub2(probs, sub3(probs, sub3(probs, 1)));
  }
  // fixed-probability bit in the reference's exact arithmetic (LzmaDec.c:325-334)
  __device__ __forceinline__ void direct(uint32_t& v) {
    norm();
    range >>= 1;
    code -= range;
    const uint32_t t = 0u - (code >> 31);
    v = (v << 1) + (t + 1u);
    code += range & t;
  }
};

// lane index within the wave (0 in the host emulation)
#ifdef LZGPU_HOST_EMU
__device__ __forceinline__ uint32_t lz_lane_id() { return 0; }
#else
__device__ __forceinline__ uint32_t lz_lane_id() { return __lane_id(); }
#endif

// Direct bits of a distance (LzmaDec.c:323-344), several per step, on the
// wave-cooperative kernel (round 4).  A direct bit reads
// no probability: NORMALIZE, range >>= 1, the bit is code >= range (the
// reference's sign trick equals the compare while code < 2^31 + range), and
// code -= range on a 1.  Between two normalisations the ranges are R >> 1,
// R >> 2, ... -- fixed before any bit is known -- and, because each is more
// than the sum of all later ones, the k bits the serial loop decodes are the
// largest v whose weight S(v) = sum over the 1-bits i of v (MSB = bit 1) of
// R >> i is <= code.  So a chunk of k <= 5 bits (k no larger than the bits the
// range allows before the next NORMALIZE: 8 - clz(R)) is decided in one step:
// lane j computes S(j), the lanes with S(j) <= code are exactly 0..v, v is
// their count - 1 (a ballot), and the winner's S is taken by readlane:
// code -= S(v), range = R >> k.  A state outside the sign trick's reach
// (code >= 2^31 + (R >> k): only a corrupt stream) takes the chunk bit by
// bit.  Returns with range >= 2^24 not guaranteed (the caller's next decision
// normalises first, as the reference does).
template <class Rd, bool U, bool F>
__device__ __forceinline__ void direct_coop(Rc<Rd, U, F>& rc, uint32_t& dist, uint32_t left) {
#ifndef LZGPU_HOST_EMU
  const uint32_t j = lz_lane_id() & 31u;
#endif
  do {
    rc.norm();
    const uint32_t R = rc.range, C = rc.code;
    uint32_t k = 8u - uint32_t(__builtin_clz(R));  // bits before the next NORMALIZE
    k = k < left ? k : left;
    k = k < 5u ? k : 5u;
    const uint32_t Rk = R >> k;
    if (C >= 0x80000000u + Rk) {
      // outside the compare's reach (corrupt input): the reference's own steps
      for (uint32_t i = 0; i < k; ++i) {
        if (i) rc.norm();
        rc.range >>= 1;
        rc.code -= rc.range;
        const uint32_t t = 0u - (rc.code >> 31);
        dist = (dist << 1) + (t + 1u);
        rc.code += rc.range & t;
      }
    } else {
#ifdef LZGPU_HOST_EMU
      uint32_t v = 0, sv = 0;
      for (uint32_t c = 0; c < (1u << k); ++c) {
        uint32_t S = 0;
        for (uint32_t t = 0; t < k; ++t)
          if ((c >> t) & 1u) S += R >> (k - t);
        if (S <= C) v = c, sv = S;
      }
#else
      // lane j's k-bit candidate: bit t of j (LSB = the chunk's last bit)
      // weighs R >> (k - t); lanes j >= 2^k hold no candidate
      uint32_t S = 0;
#pragma unroll
      for (uint32_t t = 0; t < 5u; ++t)
        S += ((j >> t) & 1u) ? (R >> ((k - t) & 31u)) : 0u;
      const bool ok = (j >> k) == 0u && S <= C;
      const uint32_t v = uint32_t(__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok))) - 1u;
      const uint32_t sv = uint32_t(__builtin_amdgcn_readlane(int(S), int(v)));
#endif
      rc.code = C - sv;
      rc.range = Rk;
      dist = (dist << k) | v;
    }
    left -= k;
  } while (left != 0);
}

// Copy n bytes of an LZ match: dic[pos..pos+n) = dic[from..], byte-serial
// overlap semantics (rep0 < n replicates the period), ring wrap at cap.
// Non-overlapping, non-wrapping spans go 8 bytes per round trip.

// Unaligned 8-byte global access (gfx950 runs global memory in unaligned
// mode: one dwordx2 per 8 bytes instead of eight byte instructions -- the
// vector-memory pipeline, not bandwidth, is what a lane's byte traffic costs).
#ifdef LZGPU_HOST_EMU
__device__ __forceinline__ uint64_t ldu64(const gbyte* p) {
  uint64_t v;
  __builtin_memcpy(&v, p, 8);
  return v;
}
__device__ __forceinline__ void stu64(gbyte* p, uint64_t v) { __builtin_memcpy(p, &v, 8); }
__device__ __forceinline__ void stu32(gbyte* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ void stu16(gbyte* p, uint32_t v) {
  const uint16_t h = uint16_t(v);
  __builtin_memcpy(p, &h, 2);
}
#else
typedef uint64_t lz_u64a1 __attribute__((aligned(1)));
typedef uint32_t lz_u32a1 __attribute__((aligned(1)));
typedef uint16_t lz_u16a1 __attribute__((aligned(1)));
__device__ __forceinline__ uint64_t ldu64(const gbyte* p) {
  return *(const __attribute__((address_space(1))) lz_u64a1*)p;
}
__device__ __forceinline__ void stu64(gbyte* p, uint64_t v) {
  *(__attribute__((address_space(1))) lz_u64a1*)p = v;
#if LZGPU_SHADOW_OUT
  *(__attribute__((address_space(1))) lz_u64a1*)(p + LZGPU_SHADOW_OUT) = v;
#endif
}
__device__ __forceinline__ void stu32(gbyte* p, uint32_t v) {
  *(__attribute__((address_space(1))) lz_u32a1*)p = v;
#if LZGPU_SHADOW_OUT
  *(__attribute__((address_space(1))) lz_u32a1*)(p + LZGPU_SHADOW_OUT) = v;
#endif
}
__device__ __forceinline__ void stu16(gbyte* p, uint32_t v) {
  *(__attribute__((address_space(1))) lz_u16a1*)p = uint16_t(v);
#if LZGPU_SHADOW_OUT
  *(__attribute__((address_space(1))) lz_u16a1*)(p + LZGPU_SHADOW_OUT) = uint16_t(v);
#endif
}
#endif
// the low rem (1..7) bytes of v to d: at most three stores
__device__ __forceinline__ void stu_tail(gbyte* d, uint64_t v, uint32_t rem) {
  if (rem & 4) {
    stu32(d, uint32_t(v));
    v >>= 32;
    d += 4;
  }
  if (rem & 2) {
    stu16(d, uint32_t(v));
    v >>= 16;
    d += 2;
  }
  if (rem & 1) lz_put(d, uint32_t(v));
}

__device__ __forceinline__ uint32_t lz_copy(gbyte* dic, uint64_t pos, uint64_t from, uint32_t n,
                                            uint32_t dist, uint64_t cap) {
  uint32_t last = 0;
  if (from + n <= cap && from < pos) {
    // source span does not wrap (always so for a flat LzmaDecode window)
    gbyte* d = dic + pos;
    const gbyte* src = dic + from;
    uint64_t v = 0;
    uint32_t i = 0;
    if (dist >= 8) {
      // src[i..i+8) lies below d + i: written before this step reads it
      for (; i + 8 <= n; i += 8) {
        v = ldu64(src + i);
        stu64(d + i, v);
      }
      if (i < n) {
        v = ldu64(src + i);
        stu_tail(d + i, v, n - i);
        return uint32_t(v >> (8 * (n - i - 1))) & 0xFFu;
      }
      return uint32_t(v >> 56);
    }
    // dist < 8: the output is src[0..dist) repeated; 8 bytes of it in v
    // (the 8-byte read stays inside the window: src + 8 <= d + 7 < cap
    // unless the match ends within 7 bytes of it)
    if (from + 8 <= cap) {
      v = ldu64(src);
      v &= ~0ull >> (64 - 8 * dist);
    } else {
      v = 0;
      for (uint32_t k = 0; k < dist; ++k) v |= uint64_t(src[k]) << (8 * k);
    }
    v |= v << (8 * dist);
    if (dist < 4) v |= v << (16 * dist);
    if (dist < 2) v |= v << 32;
    const uint32_t t = 8u % dist;  // phase advance per 8 bytes
    for (;; i += 8) {
      const uint32_t rem = n - i;
      if (rem <= 8) {
        if (rem == 8)
          stu64(d + i, v);
        else
          stu_tail(d + i, v, rem);
        return uint32_t(v >> (8 * (rem - 1))) & 0xFFu;
      }
      stu64(d + i, v);
      v = (v >> (8 * t)) | (v << (8 * (dist - t)));
    }
  }
  if (from + n <= cap) {
    gbyte* d = dic + pos;
    const gbyte* s = dic + from;
    uint32_t i = 0;
    if (dist >= 8) {
      for (; i + 8 <= n; i += 8) {
        uint8_t b0 = s[i], b1 = s[i + 1], b2 = s[i + 2], b3 = s[i + 3];
        uint8_t b4 = s[i + 4], b5 = s[i + 5], b6 = s[i + 6], b7 = s[i + 7];
        d[i] = b0; d[i + 1] = b1; d[i + 2] = b2; d[i + 3] = b3;
        d[i + 4] = b4; d[i + 5] = b5; d[i + 6] = b6; d[i + 7] = b7;
        last = b7;
      }
    }
    for (; i < n; ++i) {
      uint8_t b = s[i];
      d[i] = b;
      last = b;
    }
  } else {
    do {
      uint8_t b = dic[from];
      dic[pos++] = b;
      last = b;
      if (++from == cap) from = 0;
    } while (--n != 0);
  }
  return last;
}

// j mod d for j < 2^16, d >= 1, from the float reciprocal rd = 1/d: the
// quotient is exact or one off, corrected by one compare each way.
__device__ __forceinline__ uint32_t lz_mod_small(uint32_t j, uint32_t d, float rd) {
  const int32_t q = int32_t(float(j) * rd);
  int32_t r = int32_t(j) - q * int32_t(d);
  r += (r < 0) ? int32_t(d) : 0;
  r -= (r >= int32_t(d)) ? int32_t(d) : 0;
  return uint32_t(r);
}

// LZ copy of the wave-cooperative kernel (every lane holds the same state).
// Byte j of the match (j < n) is the window byte at from + (j mod dist) --
// written before this match, by byte-serial overlap semantics -- and the byte
// the next matched literal reads (the one at distance dist from pos + n) is
// the j = n term of the same formula.  So all of them are loaded in one batch,
// lane l taking j = l, l + 32, ...: one global round trip per 32 bytes instead
// of one per 8 bytes, and no reload of the matched byte behind the copy's own
// stores (a load waits for every earlier store in the in-order vmcnt queue).
// Lanes of one wave see each other's global stores in order (one vector L1).
// Returns the last byte copied; `mb` gets the next matched byte.
constexpr uint32_t kCoopLanes = 32u;
// Store the window's `fl` deferred bytes -- dictionary positions [end - fl,
// end), contiguous within a bulk pass -- with every lane of the wave.
__device__ __forceinline__ void win_flush(LzWin& w, gbyte* dic, uint64_t end) {
#ifdef LZGPU_HOST_EMU
  const uint32_t l0 = 0, step = 1;
#else
  const uint32_t l0 = lz_lane_id() & (kCoopLanes - 1u), step = kCoopLanes;
#endif
  for (uint32_t k = l0; k < w.fl; k += step) dic[end - w.fl + k] = w.b[(w.t - w.fl + k) & w.mask];
  w.fl = 0;
}
// WIN: the LDS history window `w` is kept up to date (every copied byte is
// also written there) and serves the loads when dist <= w.av (the byte at
// window index k of the match is at distance dist - k < dist: held).
// DEF: deferred output (def_on): the copy writes the window only.
template <bool WIN = false, bool DEF = false>
__device__ __forceinline__ uint32_t lz_copy_coop(gbyte* dic, uint64_t pos, uint64_t from,
                                                 uint32_t n, uint32_t dist, uint64_t cap,
                                                 uint32_t& mb, LzWin* w = nullptr) {
  const bool per = dist <= n;  // the match overlaps itself: period dist
#ifdef LZGPU_HOST_EMU
  // one lane plays every lane: all loads (sources lie before pos), then stores
  uint8_t v[kLenDone];  // n <= 273
  const bool inwin = WIN && dist <= w->av;
  for (uint32_t j = 0; j <= n; ++j) {
    const uint32_t k = per ? j % dist : j;
    uint64_t a = from + k;
    v[j] = inwin ? w->b[(w->t - dist + k) & w->mask] : dic[a >= cap ? a - cap : a];
  }
  if constexpr (!DEF)
    for (uint32_t j = 0; j < n; ++j) dic[pos + j] = v[j];
  if constexpr (WIN) {
    for (uint32_t j = 0; j < n; ++j) w->b[(w->t + j) & w->mask] = v[j];
    win_adv(*w, n);
  }
  if constexpr (DEF) {
    w->fl += n;
    if (w->fl >= kDeferBytes) win_flush(*w, dic, pos + n);
  }
  mb = v[n];
  return v[n - 1];
#else
  const float rd = per ? __builtin_amdgcn_rcpf(float(dist)) : 0.f;
  const uint32_t lane = lz_lane_id() & (kCoopLanes - 1u);
  // the match's index k of byte j (j <= n); j > n: a harmless in-range index
  auto k_of = [&](uint32_t j) -> uint32_t {
    return j > n ? 0u : (per ? lz_mod_small(j, dist, rd) : j);
  };
  auto src_of = [&](uint32_t j) -> uint64_t {
    const uint64_t a = from + k_of(j);
    return a >= cap ? a - cap : a;
  };
  // window-served loads: every lane decides alike (wave-uniform condition)
  const bool inwin = WIN && dist <= w->av;
  auto load = [&](uint32_t j) -> uint32_t {
    if constexpr (WIN) {
      if (inwin) return w->b[(w->t - dist + k_of(j)) & w->mask];
    }
    return dic[src_of(j)];
  };
  auto store = [&](uint32_t j, uint32_t v) {
    if constexpr (!DEF) dic[pos + j] = uint8_t(v);
    if constexpr (WIN) w->b[(w->t + j) & w->mask] = uint8_t(v);
  };
  uint32_t my_last = 0, my_mb = 0;
  // the first 64 bytes (almost every match): both loads before any store
  const uint32_t j0 = lane, j1 = lane + kCoopLanes;
  const uint32_t v0 = load(j0);
  uint32_t v1 = 0;
  if (n >= kCoopLanes) v1 = load(j1);
  if (j0 < n) store(j0, v0);
  if (j1 < n) store(j1, v1);
  my_last = (j0 + 1 == n) ? v0 : ((j1 + 1 == n) ? v1 : 0u);
  my_mb = (j0 == n) ? v0 : ((j1 == n) ? v1 : 0u);
  // longer matches: 32 bytes per round trip
  for (uint32_t b = 2 * kCoopLanes; b <= n; b += kCoopLanes) {
    const uint32_t j = b + lane;
    const uint32_t v = load(j);
    if (j < n) store(j, v);
    my_last = (j + 1 == n) ? v : my_last;
    my_mb = (j == n) ? v : my_mb;
  }
  if constexpr (WIN) {
    win_adv(*w, n);
  }
  if constexpr (DEF) {
    // (the window bytes other lanes just wrote are seen by the flush's LDS
    // reads: one wave's LDS operations complete in order)
    w->fl += n;
    if (w->fl >= kDeferBytes) win_flush(*w, dic, pos + n);
  }
  mb = uint32_t(__builtin_amdgcn_readlane(int(my_mb), int(n & (kCoopLanes - 1u))));
  return uint32_t(__builtin_amdgcn_readlane(int(my_last), int((n - 1) & (kCoopLanes - 1u))));
#endif
}

// one output byte at pos (literal / short rep), written through to the
// window where the placement has one
template <uint32_t M>
__device__ __forceinline__ void lz_emit(gbyte* dic, uint64_t pos, uint32_t v, LzWin* w) {
  lz_put(dic + pos, v);
  if constexpr (win_on<M>()) win_put(*w, v);
}

// ------------------------------------------------------------------ symbol loop

// Literal-tree cell for reference literal offset `rel` (0..0x2FF) of context ctx:
// plain part for rel < 0x100, matched part above.  Both parts in LDS (or both
// global) -> a branch-free offset select; split placement -> a real branch.
template <uint32_t M, class Lo, class Rd, bool U, bool F>
__device__ __forceinline__ uint32_t lit_bit(Rc<Rd, U, F>& rc, const Tab<M, Lo>& T, uint32_t ctx,
                                            uint32_t offs_mbit, uint32_t sym) {
  constexpr bool p_lds = ((M >> S_LITP) & 1u) != 0u, m_lds = ((M >> S_LITM) & 1u) != 0u;
  if constexpr (p_lds == m_lds) {
    const uint32_t rel = offs_mbit ? (T.L.o[S_LITM] + (ctx << 9) + offs_mbit - 0x100u)
                                   : (T.L.o[S_LITP] + (ctx << 8));
    if constexpr (p_lds)
      return rc.bit(T.lo + (rel + sym));
    else
      return rc.bit(T.g(rel + sym));
  } else {
    if (offs_mbit) return rc.bit(T.template at<S_LITM>((ctx << 9) + offs_mbit - 0x100u + sym));
    return rc.bit(T.template at<S_LITP>((ctx << 8) + sym));
  }
}

// One literal (LzmaDec.c:161-196): plain tree for state < 7, matched tree
// against the byte at rep0 otherwise; writes the byte, updates state.
template <uint32_t M, class Lo, class Rd, bool U, bool F>
__device__ __forceinline__ void lz_literal(Rc<Rd, U, F>& rc, const Tab<M, Lo>& T, uint32_t& st,
                                           uint32_t& prev, uint32_t& total, uint32_t full,
                                           uint32_t lc, uint32_t lp_mask, gbyte* dic,
                                           uint64_t& pos, uint64_t cap, uint32_t r0,
                                           uint32_t mb_pf, LzWin* w = nullptr) {
  uint32_t sym = 1;
  // (LzmaDec.c:165-166 takes context 0 before the first byte of a dictionary;
  // prev and total are 0 then, so the formula gives it without a test)
  const uint32_t ctx = ((total & lp_mask) << lc) + (prev >> (8 - lc));
  (void)full;
  constexpr bool kFuseLit = fuse_on<M>(8u) && lit_addr_on<M>() && mb_pf_on<M>() &&
                            ((M >> S_LITM) & 1u) == 0u;
  if constexpr (kFuseLit) {
    // F4 (fuse_on): an iteration in which some literal lane of the wave is
    // in a matched state -- one per pass of the symbol loop, the first after a
    // match -- takes ONE 8-level walk for all of them; every other iteration
    // is the plain walk alone.  The plain tree's address walk runs in every
    // lane: a = the plain cell of the bits decided so far, which is exactly
    // where a matched lane continues after its first mismatch (offs = 0 in the
    // reference).  While a lane is still on its matched cells its probability
    // is the preloaded pk[k] and its update goes to that global cell; its LDS
    // cell is read and written back unchanged.
    auto lp = T.template at<S_LITP>(ctx << 8);
    typedef decltype(lp) P;
    if (lz_fuse_any(st >= 7)) {
      const bool ml = st >= 7;
      st = ml ? ((st < 10) ? st - 3 : st - 6) : ((st < 4) ? 0 : st - 3);
      // a plain lane loads (and never uses) the cells of match byte 0
      const uint32_t mb = ml ? (mb_pf & 0xFFu) : 0u;
      auto lm = T.template at<S_LITM>(ctx << 9);
      uint32_t pk[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        pk[k] = lm[(((mb >> (7 - k)) & 1u) << 8) + ((1u << k) | (mb >> (8 - k)))];
      LZ_WCLS(rc, W_MLIT);
      rc.wstamp();
      constexpr lds_addr_t stp = kLdsStep<P>;
      const lds_addr_t base = lds_addr_of(lp);
      lds_addr_t k0 = lds_addr_t(0) - base, k1 = stp - base;
      lz_opaque(k1);
      lds_addr_t a = base + stp;
      bool matched = ml;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t mk = (mb >> (7 - k)) & 1u;
        if (k == 4) rd_topup_mid(*rc.rd);
        const P cell = lds_at<P>(a);
        const uint32_t pl = *cell;
        const uint32_t p = matched ? pk[k] : pl;
        rc.norm_u();
        uint16_t pn;
        const uint32_t b = rc.decide_v(p, pn) ? 1u : 0u;
        // (while matched, the symbol is the match byte's top k bits under a
        // leading 1: the cell loaded above)
        if (matched) lm[(mk << 8) + ((1u << k) | (mb >> (8 - k)))] = pn;
        *cell = matched ? uint16_t(pl) : pn;
        matched = matched && (b == mk);
        a = (a << 1) + (b ? k1 : k0);
      }
      sym = uint32_t((a - base) / stp);
    } else {
      st = (st < 4) ? 0 : st - 3;
      LZ_WCLS(rc, W_WALK);
      rc.wstamp();
      sym = rc.tree8_a(lp);
    }
  } else if (lz_br<U>(st < 7)) {
    st = (st < 4) ? 0 : st - 3;
    auto lp = T.template at<S_LITP>(ctx << 8);
    if constexpr (lit_addr_on<M>()) {
      sym = rc.tree8_a(lp);
    } else {
      const uint32_t m = rc.template tree_u<4>(lp, 1);
      rd_topup_mid(*rc.rd);
      sym = rc.template tree_u<4>(lp, m);
    }
  } else {
    uint32_t mbyte = mb_pf_on<M>() ? mb_pf : uint32_t(dic[ring_back(pos, r0, cap)]);
    st = (st < 10) ? st - 3 : st - 6;
    constexpr bool p_lds = ((M >> S_LITP) & 1u) != 0u, m_lds = ((M >> S_LITM) & 1u) != 0u;
    if constexpr (p_lds && !m_lds) {
      // While the decoded bits equal the match byte's, the cell of bit k is
      // fixed by the match byte alone (offs stays 0x100, symbol = its top k
      // bits under a leading 1): load all eight matched-tree cells at once
      // instead of one dependent global round trip per bit.  After the first
      // mismatch the walk continues in the plain tree (LDS), as the
      // reference's offs = 0 does.
      const uint32_t mb = mbyte & 0xFFu;
      auto lm = T.template at<S_LITM>(ctx << 9);
      uint32_t pk[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        pk[k] = lm[(((mb >> (7 - k)) & 1u) << 8) + ((1u << k) | (mb >> (8 - k)))];
      LZ_WCLS(rc, W_MLIT);
      rc.wstamp();
      bool matched = true;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t mk = (mb >> (7 - k)) & 1u;
        uint32_t b;
        if (k == 4) rd_topup_mid(*rc.rd);
        if (matched)
          b = rc.bit_vu(pk[k], lm + ((mk << 8) + sym));
        else
          b = rc.bit_u(T.template at<S_LITP>((ctx << 8) + sym));
        matched = matched && (b == mk);
        sym = (sym << 1) | b;
      }
    } else {
      uint32_t offs = 0x100;
      LZ_WCLS(rc, W_MLIT);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        mbyte <<= 1;
        const uint32_t mbit = mbyte & offs;
        const uint32_t b = lit_bit(rc, T, ctx, offs + mbit, sym);
        sym = (sym << 1) | b;
        offs = b ? (offs & mbit) : (offs & ~mbit);
      }
    }
  }
  prev = sym & 0xFFu;
  rd_fetch_pending(*rc.rd);
  if constexpr (def_on<M>()) {
    win_put(*w, prev);
    if (++w->fl >= kDeferBytes) win_flush(*w, dic, pos + 1);
  } else {
    lz_emit<M>(dic, pos, prev, w);
  }
  pos++;
  total++;
}

// Region timing for profiling builds (-DLZGPU_PROF=1, never the default):
// wave-uniform cycle stamps around the symbol loop's regions.
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
__device__ __forceinline__ uint64_t lz_clock() { return __builtin_amdgcn_s_memtime(); }
#define LZ_PROF_MARK(s, k, t)            \
  do {                                   \
    const uint64_t now_ = lz_clock();    \
    (s).prof[k] += now_ - (t);           \
    (t) = now_;                          \
  } while (0)
#else
#define LZ_PROF_MARK(s, k, t) ((void)0)
#endif

// any lane of the wave (the lane itself in the host emulation)
__device__ __forceinline__ bool lz_any(bool v) {
#ifdef LZGPU_HOST_EMU
  return v;
#else
  return __builtin_amdgcn_ballot_w64(v) != 0;
#endif
}


// Decode symbols until pos reaches `limit` or the reader index reaches
// `in_limit` (checked after each whole symbol; the first is always decoded).
// State is written back only on success, as LzmaDec_DecodeReal does.
template <uint32_t M, class Lo, class Rd>
__device__ __forceinline__ int lz_run(LzStateT<Lo>& s, uint64_t limit, Rd& rd,
                                      uint32_t in_limit) {
  const Tab<M, Lo> T(s);
  const uint32_t pb = s.pb;
  uint32_t st = s.st;
  uint32_t r0 = s.rep0, r1 = s.rep1, r2 = s.rep2, r3 = s.rep3;
  const uint32_t pb_mask = (1u << pb) - 1, lp_mask = (1u << s.lp) - 1;
  const uint32_t lc = s.lc;
  gbyte* __restrict__ dic = s.dic;
  const uint64_t cap = s.cap;
  uint64_t pos = s.pos;
  uint32_t total = s.total;
  const uint32_t full = s.full;
  uint32_t len = 0;
  // wave-uniform decoder state: NORMALIZE as a uniform branch (Rc), symbol
  // kinds (lz_br), the uniform symbol loop (kUL)
  constexpr bool kUN = uni_on<M>();
  constexpr bool kU = uni_on<M>();
  constexpr bool kUL = uloop_on<M>();
  Rc<Rd, kUN, bit_form<M>()> rc{s.range, s.code, &rd};
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
  rc.wacc = s.wprof;
#endif
  // previous byte (literal context), kept in a register
  uint32_t prev = 0;
  if (full != 0 || total != 0) prev = dic[(pos == 0 ? cap : pos) - 1];
  // byte at distance rep0, needed by a matched literal (state >= 7)
  uint32_t mb_pf = 0;
  if constexpr (mb_pf_on<M>()) mb_pf = (st >= 7) ? uint32_t(dic[ring_back(pos, r0, cap)]) : 0u;
  LZ_WAIT(s.wprof, W_PREV);
#ifndef LZGPU_HOST_EMU
  // Both loads complete here, before the symbol loop (round 6): a value that
  // enters the loop with its load outstanding is waited for at its use inside
  // the loop -- with vmcnt(0), i.e. behind every store in flight -- on every
  // pass, since the compiler's wait placement cannot tell the first pass from
  // the others (the one-stream kernel drained its stores at each literal).
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#endif

  uint32_t ps = 0;
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
  uint64_t t_prof = lz_clock();
#endif
#if LZGPU_PROF == 1 && !LZGPU_PROF_DRAIN && !defined(LZGPU_HOST_EMU)
  // prof[13] in the throughput placement (which writes it nowhere else): the
  // wave's time from the end of a literal batch to the next pass's start --
  // the match path -- booked by EVERY live lane, as prof[17] books the
  // iterations; prof[1] / prof[2] / prof[8..10] are summed over the lanes that
  // entered the path only, the others book the same time under prof[0]
  uint64_t t_mp = 0;
#endif
  do {
#if LZGPU_PROF == 1 && !LZGPU_PROF_DRAIN && !defined(LZGPU_HOST_EMU)
    if constexpr ((M & ~kRowBits) == LZGPU_LDS_MASK) {
      if (t_mp != 0) s.prof[13] += lz_clock() - t_mp;
    }
#endif
    uint32_t lcoder_is_rep;
    if constexpr (kUL) {
      // one symbol per pass, kind and loop exit as uniform branches
      ps = total & pb_mask;
      rd_topup(rd);
      const bool ism = rc.bit_ub(T.template at<S_MATCH>((st << pb) + ps));
      if (!lz_uni(ism)) {
        lz_literal<M>(rc, T, st, prev, total, full, lc, lp_mask, dic, pos, cap, r0, mb_pf,
                      &s.win);
        LZ_PROF_MARK(s, 0, t_prof);
        continue;
      }
      LZ_PROF_MARK(s, 0, t_prof);
    } else {
    // Up to LZGPU_LIT_BATCH symbols per pass of this loop while they are
    // literals: a lane's symbol sequence is unchanged, but lanes of a wave
    // that sit in literal runs keep decoding together instead of idling
    // behind a neighbour's match path on every symbol.
    bool is_match = false, stop = false;
    // lanes leave the batch by clearing lit_on, the loop itself exits only
    // when the whole wave is done: no divergent exit, so no per-iteration
    // copies of the lane state into exit registers
    bool lit_on = !is_match;
#pragma unroll 1
    for (int lit = 0; lit < LZGPU_LIT_BATCH; ++lit) {
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
      const uint64_t t_it = lz_clock();
#endif
#if LZGPU_PROF == 2 && !defined(LZGPU_HOST_EMU)
      {
        const uint64_t on = __builtin_amdgcn_ballot_w64(lit_on);
        const uint64_t ml = __builtin_amdgcn_ballot_w64(lit_on && st >= 7);
        s.prof[5] += 1;
        s.prof[6] += __builtin_popcountll(on);
        s.prof[7] += __builtin_popcountll(ml);
        s.prof[8] += (ml != 0 && ml != on) ? 1 : 0;
        s.prof[11] += __builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
      }
#endif
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
      const uint64_t tA = lz_clock();
      uint64_t tB = 0, tC = 0;
      bool did_lit = false;
#endif
      if (lz_br<kU>(lit_on)) {
        ps = total & pb_mask;
        rd_topup(rd);
        const uint32_t ism = rc.bit_u(T.template at<S_MATCH>((st << pb) + ps));
        if (lz_br<kU>(ism != 0)) {
          is_match = true;
          lit_on = false;
        } else {
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
          tB = lz_clock();
          did_lit = true;
#endif
          lz_literal<M>(rc, T, st, prev, total, full, lc, lp_mask, dic, pos, cap, r0, mb_pf,
                        &s.win);
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
          tC = lz_clock();
#endif
          if (lz_br<kU>(!(pos < limit && rd.used() < in_limit))) {
            stop = true;
            lit_on = false;
          }
        }
      }
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
      {
        const uint64_t tD = lz_clock();
        if (did_lit) {
          s.prof[14] += tB - tA;
          s.prof[15] += tC - tB;
          s.prof[16] += tD - tC;
        }
      }
      {
        const bool more = lz_any(lit_on);
        s.prof[17] += lz_clock() - t_it;  // the whole iteration, every live lane
        if (!more) break;
      }
#else
      if (!lz_any(lit_on)) break;
#endif
    }
    LZ_PROF_MARK(s, 0, t_prof);
#if LZGPU_PROF == 1 && !LZGPU_PROF_DRAIN && !defined(LZGPU_HOST_EMU)
    t_mp = lz_clock();
#endif
#if LZGPU_PROF == 2 && !defined(LZGPU_HOST_EMU)
    {
      const uint64_t mm = __builtin_amdgcn_ballot_w64(is_match && !stop);
      s.prof[9] += mm ? 1 : 0;
      s.prof[10] += __builtin_popcountll(mm);
      s.prof[13] += (is_match && !stop) ? 1 : 0;
    }
#endif
    if (stop) break;
    if (!is_match) continue;
    }
    LZ_WAIT(s.wprof, W_DRAIN);  // wait attribution: the stores queued so far
    LZ_WCLS(rc, W_REP);
    // Under the uniform loop the match path has no exit of its own: a short
    // rep, the end marker and a data error set xc and skip the rest of the
    // symbol, and the loop leaves at one uniform test after it.
    // Exits from inside the symbol's EXEC-masked branches made the compiler
    // keep a per-lane "which way out" value, its lane masks and copies of the
    // decoder state on every pass (~17 vector + ~30 scalar instructions per
    // literal in the one-stream kernel).  Elsewhere xc stays 0 and the exits
    // are the reference's own returns.
    uint32_t xc = 0;  // 1: short rep done, 2: end marker, 3: data error
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
#if LZGPU_PROF_DRAIN
    {
      // how long the outstanding vector-memory operations take to drain here
      const uint64_t td = lz_clock();
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      s.prof[13] += lz_clock() - td;
    }
#endif
    const uint64_t tm0 = lz_clock();
#endif
    const uint32_t is_rep = rc.bit(T.template at<S_REP>(st));
    // the length front's cells (mp_on 1): choice, choice2, the low and the mid
    // tree of this posState on the lane's coder base
    uint32_t lf_ch = 0, lf_ch2 = 0, lf_lo[7], lf_mid[7];
    if constexpr (mp_on<M>(1u)) {
      // Loaded here, ahead of the rep-distance bits: those decide and store
      // cells of IsRepG0..G2 (LDS) and IsRep0Long (its own global section)
      // only, and every path from here to the length coder makes no other
      // decision, so no store can reach a Len / RepLen cell before its use.
      // A lane that leaves before the length coder (short rep, data error)
      // has loaded sixteen cells of its own RepLen column for nothing.
      auto lb = T.g(is_rep ? T.L.o[S_REPLEN] : T.L.o[S_LEN]);
      lf_ch = lb[0];
      lf_ch2 = lb[1];
      rc.load7(lb + 2 + (ps << 3), 1, lf_lo);
      rc.load7(lb + 2 + (8u << pb) + (ps << 3), 1, lf_mid);
      LZ_WCLS(rc, W_LEN);
      rc.wstamp();
      LZ_WCLS(rc, W_REP);
    }
    if (lz_br<kU>(!is_rep)) {
      st += 12;
      lcoder_is_rep = 0;
    } else {
      if constexpr (kUL) {
        xc = (full == 0 && total == 0) ? 3u : 0u;
      } else {
        if (full == 0 && total == 0) return kErrData;
      }
      if (!kUL || xc == 0) {
      if (lz_br<kU>(!rc.bit(T.template at<S_REP>(12 + st)))) {
        if (lz_br<kU>(!rc.bit(T.template at<S_REP0L>((st << pb) + ps)))) {
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
          LZ_WAIT(s.wprof, W_DRAIN);
          const uint64_t tc0 = lz_clock();
#endif
          if constexpr ((M & kCoopBit) != 0u) {
            // short rep = a one-byte copy: the byte and the next matched byte
            // in one load batch
            prev = lz_copy_coop<win_on<M>(), def_on<M>()>(dic, pos, ring_back(pos, r0, cap), 1,
                                                          r0, cap, mb_pf, &s.win);
            pos++;
          } else {
            prev = dic[ring_back(pos, r0, cap)];
            lz_put(dic + pos++, prev);
            if constexpr (mb_pf_on<M>()) mb_pf = dic[ring_back(pos, r0, cap)];
          }
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
          __builtin_amdgcn_s_waitcnt(0x0F70);
          s.wprof[W_COPY] += lz_clock() - tc0;
#endif
          total++;
          st = (st < 7) ? 9 : 11;
          if constexpr (kUL)
            xc = 1;
          else
            continue;
        }
      } else {
        uint32_t dist;
        if (lz_br<kU>(!rc.bit(T.template at<S_REP>(24 + st)))) {
          dist = r1;
        } else {
          if (lz_br<kU>(!rc.bit(T.template at<S_REP>(36 + st)))) {
            dist = r2;
          } else {
            dist = r3;
            r3 = r2;
          }
          r2 = r1;
        }
        r1 = r0;
        r0 = dist;
      }
      if (!kUL || xc == 0) {
        st = (st < 7) ? 8 : 11;
        lcoder_is_rep = 1;
      }
      }
    }
    if (!kUL || xc == 0) {
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
    const uint64_t tm1 = lz_clock();
    s.prof[8] += tm1 - tm0;
#endif
    {
      // length coder of this match kind (LzmaDec.c:261-292)
      LZ_WCLS(rc, W_LEN);
      const uint32_t lsec_o = lcoder_is_rep ? T.L.o[S_REPLEN] : T.L.o[S_LEN];
      static_assert(((M >> S_LEN) & 1u) == ((M >> S_REPLEN) & 1u), "Len/RepLen placement");
      constexpr bool len_lds = ((M >> S_LEN) & 1u) != 0u;
      auto lbase = [&]() {
        if constexpr (len_lds) return T.lo + lsec_o; else return T.g(lsec_o);
      }();
      if constexpr (!len_lds) {
        // global length coder: the choice bits and the low tree load together,
        // the mid tree only behind choice = 1
        if constexpr ((M & ~kRowBits) != LZGPU_LDS_MASK) {
        // choice, choice2 and both 3-level trees of this posState in ONE load
        // batch; only lengths >= 18 go back to memory (LenHigh, 3 batches)
        auto lo_t = lbase + 2 + (ps << 3);
        auto mid_t = lbase + 2 + (8u << pb) + (ps << 3);
        const uint32_t ch = lbase[0], ch2 = lbase[1];
        uint32_t clo[7], cmid[7];
        rc.load7(lo_t, 1, clo);
        rc.load7(mid_t, 1, cmid);
        rc.wstamp();
        if (!rc.bit_v(ch, lbase))
          len = rc.dec3(lo_t, 1, clo) - 8;
        else if (!rc.bit_v(ch2, lbase + 1))
          len = rc.dec3(mid_t, 1, cmid);
        else {
          LZ_WCLS(rc, W_LENHI);
          len = 16 + rc.tree8_g(T.template at<S_LENHI>(lcoder_is_rep << 8)) - 256;
        }
        } else if constexpr (mp_on<M>(1u)) {
        // the length front from the batch issued at IsRep: choice, choice2
        // behind choice = 1, then F1's ONE 3-level walk for every lane with a
        // short length, its seven cells selected from the low or the mid tree
        const uint32_t c1 = rc.bit_v(lf_ch, lbase);
        uint32_t c2 = 0;
        if (c1) c2 = rc.bit_v(lf_ch2, lbase + 1);
        if (!c2) {
          auto len_t = lbase + (2 + (c1 ? (8u << pb) : 0u) + (ps << 3));
          auto pick = [&](int k) {
            const uint32_t vm = lf_mid[k], vl = lf_lo[k];
            return c1 ? vm : vl;
          };
          len = (c1 ? 8u : 0u) + rc.dec3_v(len_t, 1, pick(0), pick(1), pick(2), pick(3), pick(4),
                                           pick(5), pick(6)) - 8;
        } else {
          LZ_WCLS(rc, W_LENHI);
          if constexpr (mp_on<M>(2u))
            len = 16 + rc.tree8_g(T.template at<S_LENHI>(lcoder_is_rep << 8)) - 256;
          else
            len = 16 + rc.template tree<8>(T.template at<S_LENHI>(lcoder_is_rep << 8));
        }
        } else if constexpr (fuse_on<M>(1u)) {
        // F1: choice, then choice2 for the lanes behind choice = 1, then ONE
        // 3-level walk for every lane with a short length -- the low tree or
        // the mid tree by a per-lane base and offset
        const uint32_t ch = lbase[0];
        rc.wstamp();
        const uint32_t c1 = rc.bit_v(ch, lbase);
        uint32_t c2 = 0;
        if (c1) c2 = rc.bit(lbase + 1);
        if (!c2) {
          auto len_t = lbase + (2 + (c1 ? (8u << pb) : 0u) + (ps << 3));
          len = (c1 ? 8u : 0u) + rc.sub3(len_t, 1) - 8;
        } else {
          LZ_WCLS(rc, W_LENHI);
          if constexpr (mp_on<M>(2u))
            len = 16 + rc.tree8_g(T.template at<S_LENHI>(lcoder_is_rep << 8)) - 256;
          else
            len = 16 + rc.template tree<8>(T.template at<S_LENHI>(lcoder_is_rep << 8));
        }
        } else {
        const uint32_t ch = lbase[0];
        auto lo_t = lbase + 2 + (ps << 3);
        rc.wstamp();
        if (!rc.bit_v(ch, lbase))
          len = rc.sub3(lo_t, 1) - 8;
        else if (!rc.bit(lbase + 1))
          len = 8 + rc.sub3(lbase + 2 + (8u << pb) + (ps << 3), 1) - 8;
        else {
          LZ_WCLS(rc, W_LENHI);
          if constexpr (mp_on<M>(2u))
            len = 16 + rc.tree8_g(T.template at<S_LENHI>(lcoder_is_rep << 8)) - 256;
          else
            len = 16 + rc.template tree<8>(T.template at<S_LENHI>(lcoder_is_rep << 8));
        }
        }
      } else {
        if (lz_br<kU>(!rc.bit(lbase)))
          len = rc.template tree<3>(lbase + 2 + (ps << 3));
        else if (lz_br<kU>(!rc.bit(lbase + 1)))
          len = 8 + rc.template tree<3>(lbase + 2 + (8u << pb) + (ps << 3));
        else {
          LZ_WCLS(rc, W_LENHI);
          len = 16 + rc.template tree<8>(T.template at<S_LENHI>(lcoder_is_rep << 8));
        }
      }
    }

#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
    const uint64_t tm2 = lz_clock();
    s.prof[9] += tm2 - tm1;
#endif
    if (lz_br<kU>(st >= 12)) {
      const uint32_t lstate = len < 4 ? len : 3;
      uint32_t dist;
      LZ_WCLS(rc, W_SLOT);
      if constexpr (((M >> S_SLOT) & 1u) == 0u) {
        auto sl_t = T.template at<S_SLOT>(lstate << 6);
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
        // one global round trip + 3 decisions, timed (profiling builds)
        const uint64_t t0 = lz_clock();
        const uint32_t n1 = rc.sub3(sl_t, 1);
        const uint64_t t1 = lz_clock();
        dist = rc.sub3(sl_t, n1) - 64;
        s.prof[5] += t1 - t0;
        s.prof[6] += lz_clock() - t1;
        s.prof[7] += 1;
#else
        dist = rc.sub3(sl_t, rc.sub3(sl_t, 1)) - 64;
#endif
      } else {
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
        const uint64_t t0 = lz_clock();
        dist = rc.template tree<6>(T.template at<S_SLOT>(lstate << 6));
        s.prof[5] += lz_clock() - t0;  // slot tree (LDS placements)
#else
        dist = rc.template tree<6>(T.template at<S_SLOT>(lstate << 6));
#endif
      }
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
      const uint64_t t_tail = lz_clock();
#endif
      if (lz_br<kU>(dist >= 4)) {
        const uint32_t slot = dist;
        uint32_t nbits = (slot >> 1) - 1;
        dist = 2 | (slot & 1);
        constexpr bool kFuseTail = fuse_on<M>(2u) && ((M >> S_SPEC) & 1u) == 0u &&
                                   ((M >> S_ALIGN) & 1u) == 0u;
        if constexpr (kFuseTail) {
          // F2: the direct bits first (slot >= 14), then ONE reverse-tree walk
          // for every lane on a per-lane (base, bit count): SpecPos with
          // (slot >> 1) - 1 bits, or Align with 4 -- three levels from one load
          // batch where the lane has that many, the rest one by one
          const bool spec = slot < 14;
          uint32_t rb_off, rb_n;
          uint32_t rb_c[7];
          if constexpr (mp_on<M>(4u)) {
            // The walk's first batch issued before the direct bits: the base
            // is known with the slot (SpecPos + sp, or Align), and the direct
            // bits decide no adaptive cell, so nothing is stored between this
            // load and its use.  Seven cells from any SpecPos base stay inside
            // the SpecPos section (the last base is 82 of 114 cells); lanes
            // with slot < 4 are not here.
            rc.load7(T.g(spec ? T.L.o[S_SPEC] + ((dist << nbits) - slot - 1) : T.L.o[S_ALIGN]), 1,
                     rb_c);
          }
          if (!spec) {
            nbits -= 4;
            do rc.direct(dist); while (--nbits != 0);
            dist <<= 4;
            rb_off = T.L.o[S_ALIGN];
            rb_n = 4;
          } else {
            dist <<= nbits;
            rb_off = T.L.o[S_SPEC] + (dist - slot - 1);
            rb_n = nbits;
          }
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
          const uint64_t t_al = lz_clock();
          s.prof[6] += t_al - t_tail;  // direct bits
#endif
          LZ_WCLS(rc, W_SPEC);
          auto rb_t = T.g(rb_off);
          uint32_t mask = 1, node = 1;
          if (rb_n >= 3) {
            if constexpr (mp_on<M>(4u))
              node = rc.dec3_v(rb_t, 1, rb_c[0], rb_c[1], rb_c[2], rb_c[3], rb_c[4], rb_c[5],
                               rb_c[6]);
            else
              node = rc.sub3(rb_t, 1);
            dist |= ((node >> 2) & 1u) | (((node >> 1) & 1u) << 1) | ((node & 1u) << 2);
            mask = 8;
            rb_n -= 3;
          }
          if constexpr (mp_on<M>(4u)) {
            // the last one or two levels (two: SpecPos with 2 or 5 bits) from
            // one batch -- sub2's cells, where a lane with one level left
            // loads its node's cell three times instead of children it has
            // not got (Align ends at cell 15).  The children are other cells
            // than the node, so the first decision's store does not reach them.
            if (rb_n != 0) {
              const bool two = rb_n == 2;
              const uint32_t p0 = rb_t[node];
              const uint32_t p1 = rb_t[two ? 2 * node : node];
              const uint32_t p2 = rb_t[two ? 2 * node + 1 : node];
              rc.wstamp();
              const uint32_t b0 = rc.bit_v(p0, rb_t + node);
              node = (node << 1) | b0;
              dist |= b0 ? mask : 0u;
              if (two) {
                const uint32_t b1 = rc.bit_v(b0 ? p2 : p1, rb_t + node);
                dist |= b1 ? (mask << 1) : 0u;
              }
              rb_n = 0;
            }
          }
          while (rb_n != 0) {
            const uint32_t b = rc.bit(rb_t + node);
            node = (node << 1) | b;
            dist |= b ? mask : 0u;
            mask <<= 1;
            --rb_n;
          }
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
          s.prof[7] += lz_clock() - t_al;  // the fused SpecPos / Align walk
#endif
          if (!spec && dist == 0xFFFFFFFFu) {
            len += kLenDone;
            st -= 12;
            break;
          }
        } else if (lz_br<kU>(slot < 14)) {
          dist <<= nbits;
          uint32_t mask = 1, node = 1;
          const uint32_t sp = dist - slot - 1;
          LZ_WCLS(rc, W_SPEC);
          if constexpr (((M >> S_SPEC) & 1u) == 0u) {
            if (nbits >= 3) {
              // first three reverse-tree bits in one load batch
              node = rc.sub3(T.template at<S_SPEC>(sp), 1);
              dist |= ((node >> 2) & 1u) | (((node >> 1) & 1u) << 1) | ((node & 1u) << 2);
              mask = 8;
              nbits -= 3;
            }
            if constexpr ((M & ~kRowBits) != LZGPU_LDS_MASK) if (nbits == 2) {
              // the last two bits in one batch as well
              const uint32_t n2 = rc.sub2(T.template at<S_SPEC>(sp), node);
              dist |= (((n2 >> 1) & 1u) ? mask : 0u) | ((n2 & 1u) ? (mask << 1) : 0u);
              nbits = 0;
            }
          }
          while (lz_br<kU>(nbits != 0)) {
            uint32_t b = rc.bit(T.template at<S_SPEC>(sp + node));
            node = (node << 1) | b;
            dist |= b ? mask : 0u;
            mask <<= 1;
            --nbits;
          }
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
          s.prof[13] += lz_clock() - t_tail;  // SpecPos bits
#endif
        } else {
          nbits -= 4;
          if constexpr ((M & kCoopBit) != 0u && kDirectChunks)
            direct_coop(rc, dist, nbits);
          else
            do rc.direct(dist); while (--nbits != 0);
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
          const uint64_t t_al = lz_clock();
          s.prof[6] += t_al - t_tail;  // direct bits
#endif
          dist <<= 4;
          uint32_t node = 1;
          LZ_WCLS(rc, W_ALIGN);
          if constexpr (((M >> S_ALIGN) & 1u) == 0u) {
            if constexpr ((M & ~kRowBits) != LZGPU_LDS_MASK) {
              // all four reverse bits from one batch of the 15 cells
              node = rc.sub4(T.template at<S_ALIGN>(0), 1);
              dist |= ((node >> 3) & 1u) | (((node >> 2) & 1u) << 1) |
                      (((node >> 1) & 1u) << 2) | ((node & 1u) << 3);
            } else {
              node = rc.sub3(T.template at<S_ALIGN>(0), 1);
              dist |= ((node >> 2) & 1u) | (((node >> 1) & 1u) << 1) | ((node & 1u) << 2);
              const uint32_t b = rc.bit(T.template at<S_ALIGN>(node));
              dist |= b << 3;
            }
          } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
              uint32_t b = rc.bit(T.template at<S_ALIGN>(node));
              node = (node << 1) | b;
              dist |= b << k;
            }
          }
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
          s.prof[7] += lz_clock() - t_al;  // align bits
#endif
          if (dist == 0xFFFFFFFFu) {
            len += kLenDone;
            st -= 12;
            if constexpr (kUL)
              xc = 2;
            else
              break;
          }
        }
      }
      if (!kUL || xc == 0) {
      r3 = r2;
      r2 = r1;
      r1 = r0;
      r0 = dist + 1;
      if (full == 0 ? dist >= total : dist >= full) {
        if constexpr (kUL)
          xc = 3;
        else
          return kErrData;
      }
      st = (st < 19) ? 7 : 10;
      }
#if LZGPU_PROF == 1 && !defined(LZGPU_HOST_EMU)
      s.prof[10] += lz_clock() - tm2;
      s.prof[11] += 1;
#endif
    }
    if (!kUL || xc == 0) {
    len += 2;
    LZ_PROF_MARK(s, 1, t_prof);
    if (limit == pos) {
      if constexpr (kUL)
        xc = 3;
      else
        return kErrData;
    }
    }
    if (!kUL || xc == 0) {
      const uint64_t room = limit - pos;
      const uint32_t n = (room < len) ? uint32_t(room) : len;
      const uint64_t from = ring_back(pos, r0, cap);
      total += n;
      len -= n;
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
      LZ_WAIT(s.wprof, W_DRAIN);  // the match path's table updates
      const uint64_t tc0 = lz_clock();
#endif
      if constexpr ((M & kCoopBit) != 0u) {
        prev = lz_copy_coop<win_on<M>(), def_on<M>()>(dic, pos, from, n, r0, cap, mb_pf, &s.win);
        pos += n;
      } else {
        prev = lz_copy(dic, pos, from, n, r0, cap);
        pos += n;
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
        __builtin_amdgcn_s_waitcnt(0x0F70);
        s.wprof[W_COPY] += lz_clock() - tc0;
#endif
        if constexpr (mb_pf_on<M>()) mb_pf = dic[ring_back(pos, r0, cap)];
        LZ_WAIT(s.wprof, W_MB);
      }
#if LZGPU_PROF == 3 && !defined(LZGPU_HOST_EMU)
      if constexpr ((M & kCoopBit) != 0u) {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        s.wprof[W_COPY] += lz_clock() - tc0;
      }
#endif
    }
    }  // !kUL || xc == 0: length, distance, copy
    LZ_PROF_MARK(s, 2, t_prof);
    if constexpr (kUL) {
      if (lz_uni(xc >= 2u)) {
        if (lz_uni(xc == 3u)) return kErrData;
        break;  // the end marker
      }
    }
  } while (kUL ? lz_uni(pos < limit && rd.used() < in_limit) : (pos < limit && rd.used() < in_limit));

  if constexpr (def_on<M>()) win_flush(s.win, dic, pos);  // the dictionary complete again
  rc.norm();
  s.range = rc.range;
  s.code = rc.code;
  s.pending = len;
  s.pos = pos;
  s.total = total;
  s.rep0 = r0;
  s.rep1 = r1;
  s.rep2 = r2;
  s.rep3 = r3;
  s.st = st;
  return kOk;
}

template <uint32_t M = 0u, class Lo>
__device__ __forceinline__ void lz_flush_pending(LzStateT<Lo>& s, uint64_t limit) {
  if (s.pending == 0 || s.pending >= kLenDone) return;
  uint32_t n = s.pending;
  if (limit - s.pos < n) n = uint32_t(limit - s.pos);
  if (s.full == 0 && s.dict_size - s.total <= n) s.full = s.dict_size;
  s.total += n;
  s.pending -= n;
  while (n-- != 0) {
    const uint8_t b = s.dic[ring_back(s.pos, s.rep0, s.cap)];
    s.dic[s.pos] = b;
    if constexpr (win_on<M>()) win_put(s.win, b);
    s.pos++;
  }
}

template <uint32_t M, class Lo, class Rd>
__device__ __forceinline__ int lz_run_split(LzStateT<Lo>& s, uint64_t limit, Rd& rd,
                                            uint32_t in_limit) {
  do {
    uint64_t lim = limit;
    if (s.full == 0) {
      uint32_t left = s.dict_size - s.total;
      if (limit - s.pos > left) lim = s.pos + left;
    }
    if (lz_run<M>(s, lim, rd, in_limit) != kOk) return kErrData;
    if (s.total >= s.dict_size) s.full = s.dict_size;
    lz_flush_pending<M>(s, limit);
  } while (s.pos < limit && rd.used() < in_limit && s.pending < kLenDone);
  if (s.pending > kLenDone) s.pending = kLenDone;
  return kOk;
}

// ------------------------------------------------------------------ look-ahead dry run

enum : int { PROBE_SHORT = 0, PROBE_LIT = 1, PROBE_MATCH = 2, PROBE_REP = 3 };

template <class BP>
struct Probe {
  uint32_t range, code;
  BP in;
  BP end;
  __device__ __forceinline__ bool norm() {
    if (range < kTop) {
      if (in >= end) return false;
      range <<= 8;
      code = (code << 8) | *in++;
    }
    return true;
  }
  // 0/1, or -1 when the input ran out
  template <class P>
  __device__ __forceinline__ int bit(P prob) {
    if (!norm()) return -1;
    uint32_t bound = (range >> 11) * uint32_t(*prob);
    if (code < bound) { range = bound; return 0; }
    range -= bound;
    code -= bound;
    return 1;
  }
  template <class P>
  __device__ __forceinline__ bool tree(P probs, uint32_t bits, uint32_t& out) {
    uint32_t m = 1, lim = 1u << bits;
    while (m < lim) {
      int b = bit(probs + m);
      if (b < 0) return false;
      m = (m << 1) | uint32_t(b);
    }
    out = m - lim;
    return true;
  }
};

// Would one more symbol decode from [in, in+n)?  (LzmaDec_TryDummy)
template <uint32_t M, class Lo, class BP>
__device__ int lz_probe(const LzStateT<Lo>& s, BP in, uint64_t n) {
  const Tab<M, Lo> T(s);
  const uint32_t pb = s.pb;
  const uint32_t ps = s.total & ((1u << pb) - 1);
  uint32_t st = s.st, is_rep, len = 0;
  int kind, b;
  Probe<BP> t{s.range, s.code, in, in + n};
#define LZ_PB(p) do { b = t.bit(p); if (b < 0) return PROBE_SHORT; } while (0)
  LZ_PB(T.template at<S_MATCH>((st << pb) + ps));
  if (b == 0) {
    uint32_t sym = 1, ctx = 0;
    if (s.full != 0 || s.total != 0) {
      uint32_t prev = s.dic[(s.pos == 0 ? s.cap : s.pos) - 1];
      ctx = ((s.total & ((1u << s.lp) - 1)) << s.lc) + (prev >> (8 - s.lc));
    }
    if (st < 7) {
      while (sym < 0x100) {
        LZ_PB(T.template at<S_LITP>((ctx << 8) + sym));
        sym = (sym << 1) | uint32_t(b);
      }
    } else {
      uint32_t mbyte = s.dic[ring_back(s.pos, s.rep0, s.cap)];
      uint32_t offs = 0x100;
      while (sym < 0x100) {
        mbyte <<= 1;
        const uint32_t mbit = mbyte & offs;
        if (offs + mbit)
          LZ_PB(T.template at<S_LITM>((ctx << 9) + offs + mbit - 0x100u + sym));
        else
          LZ_PB(T.template at<S_LITP>((ctx << 8) + sym));
        sym = (sym << 1) | uint32_t(b);
        offs = b ? (offs & mbit) : (offs & ~mbit);
      }
    }
    kind = PROBE_LIT;
  } else {
    LZ_PB(T.template at<S_REP>(st));
    if (b == 0) {
      st = 0;
      is_rep = 0;
      kind = PROBE_MATCH;
    } else {
      kind = PROBE_REP;
      LZ_PB(T.template at<S_REP>(12 + st));
      if (b == 0) {
        LZ_PB(T.template at<S_REP0L>((st << pb) + ps));
        if (b == 0) return t.norm() ? PROBE_REP : PROBE_SHORT;
      } else {
        LZ_PB(T.template at<S_REP>(24 + st));
        if (b != 0) LZ_PB(T.template at<S_REP>(36 + st));
      }
      st = 12;
      is_rep = 1;
    }
    const uint32_t lo_off = is_rep ? T.L.o[S_REPLEN] : T.L.o[S_LEN];
    auto lbase = [&]() {
      if constexpr (((M >> S_LEN) & 1u) != 0u) return T.lo + lo_off; else return T.g(lo_off);
    }();
    LZ_PB(lbase);
    if (b == 0) {
      if (!t.tree(lbase + 2 + (ps << 3), 3, len)) return PROBE_SHORT;
    } else {
      LZ_PB(lbase + 1);
      if (b == 0) {
        if (!t.tree(lbase + 2 + (8u << pb) + (ps << 3), 3, len)) return PROBE_SHORT;
        len += 8;
      } else {
        if (!t.tree(T.template at<S_LENHI>(is_rep << 8), 8, len)) return PROBE_SHORT;
        len += 16;
      }
    }
    if (st < 4) {
      uint32_t slot;
      if (!t.tree(T.template at<S_SLOT>((len < 4 ? len : 3) << 6), 6, slot)) return PROBE_SHORT;
      if (slot >= 4) {
        uint32_t nbits = (slot >> 1) - 1, node = 1;
        if (slot < 14) {
          const uint32_t sp = ((2u | (slot & 1)) << nbits) - slot - 1;
          do {
            LZ_PB(T.template at<S_SPEC>(sp + node));
            node = (node << 1) | uint32_t(b);
          } while (--nbits != 0);
        } else {
          nbits -= 4;
          do {
            if (!t.norm()) return PROBE_SHORT;
            t.range >>= 1;
            t.code -= t.range & (((t.code - t.range) >> 31) - 1);
          } while (--nbits != 0);
          nbits = 4;
          do {
            LZ_PB(T.template at<S_ALIGN>(node));
            node = (node << 1) | uint32_t(b);
          } while (--nbits != 0);
        }
      }
    }
  }
#undef LZ_PB
  return t.norm() ? kind : PROBE_SHORT;
}

// ------------------------------------------------------------------ init + driver

// All cells to 1024 (LzmaDec_InitStateReal, LzmaDec.c:707-717), both tables.
template <class P>
__device__ __forceinline__ void fill_prob_init(P p, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) p[i] = uint16_t(kProbInit);
}
#ifndef LZGPU_HOST_EMU
// The same with 16-byte stores (8 cells each) after a head of single cells up
// to the next 16-byte boundary: a 4 KiB stream's global sections are 1,458
// cells, one store instruction per cell was ~10 % of the kernel's instructions.
typedef unsigned int lz_u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) lz_u32x4 lz_gv4;
typedef __attribute__((address_space(3))) lz_u32x4 lz_lv4;
template <class V, class P>
__device__ __forceinline__ void fill_prob_init16(P p, uint32_t n) {
  const uint32_t v = kProbInit | (kProbInit << 16);
  const lz_u32x4 w = {v, v, v, v};
  uint32_t i = 0;
  while (i < n && (reinterpret_cast<uintptr_t>(p + i) & 15u) != 0) p[i++] = uint16_t(kProbInit);
  for (; i + 8 <= n; i += 8) *reinterpret_cast<V*>(p + i) = w;
  for (; i < n; ++i) p[i] = uint16_t(kProbInit);
}
__device__ __forceinline__ void fill_prob_init(gu16* p, uint32_t n) {
  fill_prob_init16<lz_gv4>(p, n);
}
__device__ __forceinline__ void fill_prob_init(lds_u16* p, uint32_t n) {
  fill_prob_init16<lz_lv4>(p, n);
}
#endif

template <uint32_t M, class Lo>
__device__ __forceinline__ void lz_init_state_real(LzStateT<Lo>& s) {
  const Layout L = make_layout_m(s.lc, s.lp, s.pb, M);
  if constexpr ((M & kSessHybBit) != 0u) {
    // LDS sections packed, the others in place in the whole table
    fill_prob_init(s.lo, L.lds_cells);
    for (uint32_t k = 0; k < S_NSEC; ++k)
      if (!((M >> k) & 1u)) fill_prob_init(s.gl + L.o[k], sec_cells(k, s.lc, s.lp, s.pb));
    s.rep0 = s.rep1 = s.rep2 = s.rep3 = 1;
    s.st = 0;
    s.need_state_init = 0;
    return;
  }
#ifndef LZGPU_HOST_EMU
  if constexpr ((M & kCoopBit) != 0u) {
    // cooperative kernel: the lanes share the stream's tables, each fills a
    // stride (a wave's own LDS and global stores are seen by its later loads)
    for (uint32_t i = threadIdx.x; i < L.lds_cells; i += blockDim.x) s.lo[i] = uint16_t(kProbInit);
    for (uint32_t i = threadIdx.x; i < L.glb_cells; i += blockDim.x) s.gl[i] = uint16_t(kProbInit);
  } else
#endif
  {
    if constexpr (lds_ilv<M>()) {
      for (uint32_t i = 0; i < L.lds_cells; ++i) s.lo[kIlv * i] = uint16_t(kProbInit);
    } else if constexpr ((M & ~kCoopBit) != 0u) {
      fill_prob_init(s.lo, L.lds_cells);
    }
    if constexpr ((M & kIlvBit) != 0u) {
      // the lane's column: one cell per row (the lanes of a group that start
      // together store whole 64-byte rows)
      for (uint32_t i = 0; i < L.glb_cells; ++i) s.gl[kIlv * i] = uint16_t(kProbInit);
    } else {
      fill_prob_init(s.gl, L.glb_cells);
    }
  }
  s.rep0 = s.rep1 = s.rep2 = s.rep3 = 1;
  s.st = 0;
  s.need_state_init = 0;
}

template <class Lo>
__device__ __forceinline__ void lz_init_dic_state(LzStateT<Lo>& s, bool init_dic,
                                                  bool init_state) {
  s.need_rc_init = 1;
  s.pending = 0;
  s.tmp_n = 0;
  if (init_dic) {
    s.total = 0;
    s.full = 0;
    s.need_state_init = 1;
  }
  if (init_state) s.need_state_init = 1;
}

// LzmaDec_DecodeToDic for one lane.  src is global memory.  WithTemp = false
// drops the tempBuf continuation path, which a one-call decode (all input
// present) never takes: its first need is a NEEDS_MORE_INPUT return.
// fast_tail (one-shot decodes only): the last < 20 input bytes are decoded in
// one bulk pass, checked afterwards, instead of one symbol per pass behind the
// reference's look-ahead probe (LzmaDec.c:775-800, LzmaDec_TryDummy).  A
// symbol the probe lets through is one whose reads, plus the byte a following
// NORMALIZE would take, stay inside the input; reads only grow, so checking
// the pass's last symbol checks them all.  If that fails, or the pass stops on
// a data error (which may sit in a symbol the probe would have refused), it
// returns kRetryExact and the caller decodes the item again on the exact path.
template <bool WithTemp, uint32_t M, class Lo>
__device__ __forceinline__ int lz_decode_to_dic(LzStateT<Lo>& s, uint64_t dic_limit,
                                                const gbyte* src, uint64_t& src_len, int fin,
                                                int& status, bool fast_tail = false) {
  uint64_t avail = src_len;
  src_len = 0;
  lz_flush_pending<M>(s, dic_limit);
  status = kStNone;

  while (s.pending != kLenDone) {
    bool at_end_check = false;
    if (s.need_rc_init) {
      while (avail > 0 && s.tmp_n < 5) {
        s.tmp.set(s.tmp_n++, *src++);
        src_len++;
        avail--;
      }
      if (s.tmp_n < 5) { status = kStMoreInput; return kOk; }
      if (s.tmp.get(0) != 0) return kErrData;
      s.code = (s.tmp.get(1) << 24) | (s.tmp.get(2) << 16) | (s.tmp.get(3) << 8) | s.tmp.get(4);
      s.range = 0xFFFFFFFFu;
      s.need_rc_init = 0;
      s.tmp_n = 0;
    }
    if (s.pos >= dic_limit) {
      if (s.pending == 0 && s.code == 0) { status = kStMaybeDone; return kOk; }
      if (fin == kFinAny) { status = kStNotDone; return kOk; }
      if (s.pending != 0) { status = kStNotDone; return kErrData; }
      at_end_check = true;
    }
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
    const uint64_t t_init = lz_clock();
    if (s.need_state_init) lz_init_state_real<M>(s);
    s.prof[20] += lz_clock() - t_init;
#else
    if (s.need_state_init) lz_init_state_real<M>(s);
#endif

    if (!WithTemp || s.tmp_n == 0) {
      uint32_t in_limit;
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
      const uint64_t t_tail = lz_clock();
      const bool tail = avail < kLookahead || at_end_check;
#endif
      const bool fast = !WithTemp && fast_tail && avail < kLookahead && avail != 0 && !at_end_check;
      if (fast) {
        in_limit = uint32_t(avail);  // through the last byte, checked below
      } else if (avail < kLookahead || at_end_check) {
        int k = lz_probe<M>(s, src, avail);
        if (k == PROBE_SHORT) {
          for (uint32_t i = 0; i < uint32_t(avail); ++i) s.tmp.set(i, src[i]);
          s.tmp_n = uint32_t(avail);
          src_len += avail;
          status = kStMoreInput;
          return kOk;
        }
        if (at_end_check && k != PROBE_MATCH) { status = kStNotDone; return kErrData; }
        in_limit = 0;
      } else {
        uint64_t lim = avail - kLookahead;
        in_limit = lim > 0xFFFFFFF0ull ? 0xFFFFFFF0u : uint32_t(lim);
      }
      typename BulkReaderFor<M>::type rd;
      rd.init(src, avail);
      const int rr = lz_run_split<M>(s, dic_limit, rd, in_limit);
#if LZGPU_PROF && !defined(LZGPU_HOST_EMU)
#if LZGPU_PROF == 3
      s.wprof[W_INPUT] += rd.prof;
      if constexpr (kIsQ<typename BulkReaderFor<M>::type>) s.wprof[W_FETCH] += rd.prof_fetch;
#else
      s.prof[4] += rd.prof;
#endif
      if (tail) {
        s.prof[18] += lz_clock() - t_tail;
        s.prof[19] += 1;
      }
#endif
      // the probe also wants the byte the next NORMALIZE would take
      // (LzmaDec_TryDummy ends in NORMALIZE_CHECK); a data error may sit in a
      // symbol the probe would have refused: both go exact
      if (fast && (rr != kOk || uint64_t(rd.used()) + (s.range < kTop ? 1u : 0u) > avail))
        return kRetryExact;
      if (rr != kOk) return kErrData;
      const uint32_t used = rd.used();
      src_len += used;
      src += used;
      avail -= used;
    } else {
      uint32_t have = s.tmp_n, taken = 0;
      while (have < kLookahead && taken < avail) s.tmp.set(have++, src[taken++]);
      s.tmp_n = have;
      if (have < kLookahead || at_end_check) {
        int k = lz_probe<M>(s, LzTmpIter{s.tmp, 0u}, have);
        if (k == PROBE_SHORT) {
          src_len += taken;
          status = kStMoreInput;
          return kOk;
        }
        if (at_end_check && k != PROBE_MATCH) { status = kStNotDone; return kErrData; }
      }
      LocalReader rd;
      rd.init(s.tmp);
      if (lz_run_split<M>(s, dic_limit, rd, 0) != kOk) return kErrData;
      taken -= (have - rd.used());
      src_len += taken;
      src += taken;
      avail -= taken;
      s.tmp_n = 0;
    }
  }
  if (s.code == 0) status = kStDoneMark;
  return s.code == 0 ? kOk : kErrData;
}

// ------------------------------------------------------------------ props

__device__ __host__ inline int lz_props_parse(const uint8_t* b, uint32_t n, uint32_t& lc,
                                              uint32_t& lp, uint32_t& pb, uint32_t& dict) {
  if (n < 5) return kErrUnsupported;
  dict = uint32_t(b[1]) | (uint32_t(b[2]) << 8) | (uint32_t(b[3]) << 16) | (uint32_t(b[4]) << 24);
  if (dict < 4096) dict = 4096;
  uint32_t d = b[0];
  if (d >= 225) return kErrUnsupported;
  lc = d % 9;
  lp = (d / 9) % 5;
  pb = d / 45;
  return kOk;
}

}  // namespace lzgpu
