/*
 * lzma_gpu.h -- C ABI of liblzmagpu.so, the MI355X (gfx950) LZMA decoder.
 *
 * Two surfaces:
 *
 *  1. Drop-in symbols of the reference decoder (LZMA SDK 9.20, the
 *     yurket/lzma-sdk-zlibLike fork).  Same names, argument meaning, enum
 *     values, struct layouts and SRes codes, so a caller linking the
 *     reference's LzmaDec.o / LzmaLib.o / Lzma2Dec.o can link this library
 *     instead.  Decoding runs on the GPU; only property parsing and
 *     allocation bookkeeping stay on the host.
 *
 *       LzmaProps_Decode        replaces LzmaDec.h:40  / LzmaDec.c:898-922
 *       LzmaDec_AllocateProbs   replaces LzmaDec.h:134 / LzmaDec.c:938-948
 *       LzmaDec_FreeProbs       replaces LzmaDec.h:135 / LzmaDec.c:880-884
 *       LzmaDec_Allocate        replaces LzmaDec.h:137 / LzmaDec.c:950-970
 *       LzmaDec_Free            replaces LzmaDec.h:138 / LzmaDec.c:892-896
 *       LzmaDec_Init            replaces LzmaDec.h:73  / LzmaDec.c:701-705
 *       LzmaDec_DecodeToDic     replaces LzmaDec.h:181-182 / LzmaDec.c:719-838
 *       LzmaDec_DecodeToBuf     replaces LzmaDec.h:198-199 / LzmaDec.c:840-878
 *       LzmaDecode              replaces LzmaDec.h:223-225 / LzmaDec.c:972-1002
 *       LzmaUncompress          replaces LzmaLib.h:128-129 / LzmaLib.c:41-46
 *       Lzma2Dec_AllocateProbs  replaces Lzma2Dec.h:31 / Lzma2Dec.c:75-80
 *       Lzma2Dec_Allocate       replaces Lzma2Dec.h:32 / Lzma2Dec.c:82-87
 *       Lzma2Dec_Init           replaces Lzma2Dec.h:33 / Lzma2Dec.c:89-96
 *       Lzma2Dec_DecodeToDic    replaces Lzma2Dec.h:51-52 / Lzma2Dec.c:170-289
 *       Lzma2Dec_DecodeToBuf    replaces Lzma2Dec.h:54-55 / Lzma2Dec.c:291-328
 *       Lzma2Decode             replaces Lzma2Dec.h:77-78 / Lzma2Dec.c:330-356
 *       LzmaDec_InitDicAndState exported like LzmaDec.c:685 (declared by Lzma2Dec.c:168)
 *       LzmaEncProps_Init       replaces LzmaEnc.h:33 / LzmaEnc.c:45-51
 *       LzmaEncProps_Normalize  replaces LzmaEnc.h:34 / LzmaEnc.c:53-74
 *       LzmaEncProps_GetDictSize replaces LzmaEnc.h:35 / LzmaEnc.c:76-81
 *       LzmaEncode              replaces LzmaEnc.h:72-74 / LzmaEnc.c:2248-2268
 *       LzmaCompress            replaces LzmaLib.h:98-107 / LzmaLib.c:15-38
 *       LzmaEnc_Create          replaces LzmaEnc.h:52 / LzmaEnc.c:1700-1707
 *       LzmaEnc_Destroy         replaces LzmaEnc.h:53 / LzmaEnc.c:1727-1731
 *       LzmaEnc_SetProps        replaces LzmaEnc.h:54 / LzmaEnc.c:391-443
 *       LzmaEnc_WriteProperties replaces LzmaEnc.h:55 / LzmaEnc.c:2191-2218
 *       LzmaEnc_Encode          replaces LzmaEnc.h:56-57 / LzmaEnc.c:2184-2189
 *       LzmaEnc_MemEncode       replaces LzmaEnc.h:58-59 / LzmaEnc.c:2220-2246
 *                               (differences: at their declarations below)
 *       Lzma2EncProps_Init      replaces Lzma2Enc.h:21 / Lzma2Enc.c:168-174
 *       Lzma2EncProps_Normalize replaces Lzma2Enc.h:22 / Lzma2Enc.c:176-234
 *       Lzma2Enc_Create         replaces Lzma2Enc.h:38 / Lzma2Enc.c:367-387
 *       Lzma2Enc_Destroy        replaces Lzma2Enc.h:39 / Lzma2Enc.c:389-409
 *       Lzma2Enc_SetProps       replaces Lzma2Enc.h:40 / Lzma2Enc.c:411-421
 *       Lzma2Enc_WriteProperties replaces Lzma2Enc.h:41 / Lzma2Enc.c:423-432
 *       Lzma2Enc_Encode         replaces Lzma2Enc.h:42-43 / Lzma2Enc.c:434-477
 *                               (differences: at its declaration below)
 *       Lzma86_Encode           replaces Lzma86.h:71-72 / Lzma86Enc.c:17-108
 *       Lzma86_GetUnpackSize    replaces Lzma86.h:87 / Lzma86Dec.c:13-22
 *       Lzma86_Decode           replaces Lzma86.h:107 / Lzma86Dec.c:24-56
 *                               (differences: at their declarations below)
 *
 *     Encoding covers the reference's fast path (algo 0 with the hash-chain
 *     finder, what levels 0..4 select) and, once switched on with
 *     LzmaEncGpu_SetModes or LZGPU_ENC_MODES, its normal mode (the optimal
 *     parser and the Bt4 finder, levels 5..9): the output is that of the
 *     reference's single-threaded encoder, bit for bit.  Documented differences
 *     of LzmaEncode / LzmaCompress: props that normalise to a mode the mask
 *     does not allow -- with the initial mask of 0 the optimal parser (algo 1)
 *     and every bt finder (btMode 1), the default level 5 among them; with any
 *     mask Bt2 and Bt3 (numHashBytes below 4) -- return SZ_ERROR_UNSUPPORTED
 *     with nothing written, and LzmaGpu_LastError() names the props field; a
 *     source of 2^31 bytes or more
 *     returns SZ_ERROR_UNSUPPORTED; `progress` is ignored and the allocators
 *     are unused; LzmaEncProps_Normalize sets numThreads as a build with
 *     threads does, and the value is unused.
 *
 *     Documented differences: no stdout print in LzmaDec_AllocateProbs (the
 *     fork's LzmaDec.c:945 debug printf); Lzma2Decode initialises its state
 *     (the reference one-call omits Lzma2Dec_Init, which is undefined
 *     behaviour); a dicLimit beyond dicBufSize returns SZ_ERROR_PARAM instead
 *     of writing out of bounds; after an LzmaDec_DecodeToDic / DecodeToBuf call
 *     that returns SZ_ERROR_DATA, dic[dicPos, ...) keeps its previous contents
 *     (the reference leaves the failed pass's partly decoded bytes there:
 *     LzmaDec.c:366-379 returns before the dicPos write-back at :413-423; the
 *     drop-in downloads only dic[old dicPos, new dicPos) -- both are bytes past
 *     dicPos, which the reference's contract never defines); without a usable
 *     HIP device every decode entry returns SZ_ERROR_FAIL and LzmaGpu_LastError()
 *     says why (there is no CPU fallback).
 *
 *  2. The batch extension (new): many independent streams per launch, all
 *     buffers caller-owned device memory, no allocation inside the call.
 */
#ifndef LZMA_GPU_H
#define LZMA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- base ABI (Types.h:25-97,227-234) */

#ifndef SZ_OK
#define SZ_OK 0
#define SZ_ERROR_DATA 1
#define SZ_ERROR_MEM 2
#define SZ_ERROR_CRC 3
#define SZ_ERROR_UNSUPPORTED 4
#define SZ_ERROR_PARAM 5
#define SZ_ERROR_INPUT_EOF 6
#define SZ_ERROR_OUTPUT_EOF 7
#define SZ_ERROR_READ 8
#define SZ_ERROR_WRITE 9
#define SZ_ERROR_PROGRESS 10
#define SZ_ERROR_FAIL 11
#define SZ_ERROR_THREAD 12
#define SZ_ERROR_ARCHIVE 16
#define SZ_ERROR_NO_ARCHIVE 17
#endif

#ifndef __7Z_TYPES_H
typedef int SRes;
typedef unsigned char Byte;
typedef unsigned short UInt16;
typedef unsigned int UInt32;
typedef unsigned long long UInt64;
typedef size_t SizeT;
typedef int Bool;
typedef struct {
  void *(*Alloc)(void *p, size_t size);
  void (*Free)(void *p, void *address);
} ISzAlloc;
#endif

#define LZMA_PROPS_SIZE 5
#define LZMA_REQUIRED_INPUT_MAX 20

typedef UInt16 CLzmaProb; /* 16-bit probabilities (_LZMA_PROB32 not defined) */

typedef struct _CLzmaProps {
  unsigned lc, lp, pb;
  UInt32 dicSize;
} CLzmaProps;

/* Field order and types are the public layout of LzmaDec.h:50-69: callers of
 * the dictionary interface read dic/dicPos/dicBufSize directly. */
typedef struct {
  CLzmaProps prop;
  CLzmaProb *probs;
  Byte *dic;
  const Byte *buf;
  UInt32 range, code;
  SizeT dicPos;
  SizeT dicBufSize;
  UInt32 processedPos;
  UInt32 checkDicSize;
  unsigned state;
  UInt32 reps[4];
  unsigned remainLen;
  int needFlush;
  int needInitState;
  UInt32 numProbs;
  unsigned tempBufSize;
  Byte tempBuf[LZMA_REQUIRED_INPUT_MAX];
} CLzmaDec;

#define LzmaDec_Construct(p) { (p)->dic = 0; (p)->probs = 0; }

typedef enum { LZMA_FINISH_ANY, LZMA_FINISH_END } ELzmaFinishMode;

typedef enum {
  LZMA_STATUS_NOT_SPECIFIED,
  LZMA_STATUS_FINISHED_WITH_MARK,
  LZMA_STATUS_NOT_FINISHED,
  LZMA_STATUS_NEEDS_MORE_INPUT,
  LZMA_STATUS_MAYBE_FINISHED_WITHOUT_MARK
} ELzmaStatus;

/* ---------------------------------------------------------------- drop-in LzmaDec.h */

SRes LzmaProps_Decode(CLzmaProps *p, const Byte *data, unsigned size);
SRes LzmaDec_AllocateProbs(CLzmaDec *p, const Byte *props, unsigned propsSize, ISzAlloc *alloc);
void LzmaDec_FreeProbs(CLzmaDec *p, ISzAlloc *alloc);
SRes LzmaDec_Allocate(CLzmaDec *state, const Byte *prop, unsigned propsSize, ISzAlloc *alloc);
void LzmaDec_Free(CLzmaDec *state, ISzAlloc *alloc);
void LzmaDec_Init(CLzmaDec *p);
void LzmaDec_InitDicAndState(CLzmaDec *p, Bool initDic, Bool initState);
SRes LzmaDec_DecodeToDic(CLzmaDec *p, SizeT dicLimit, const Byte *src, SizeT *srcLen,
                         ELzmaFinishMode finishMode, ELzmaStatus *status);
SRes LzmaDec_DecodeToBuf(CLzmaDec *p, Byte *dest, SizeT *destLen, const Byte *src,
                         SizeT *srcLen, ELzmaFinishMode finishMode, ELzmaStatus *status);
SRes LzmaDecode(Byte *dest, SizeT *destLen, const Byte *src, SizeT *srcLen,
                const Byte *propData, unsigned propSize, ELzmaFinishMode finishMode,
                ELzmaStatus *status, ISzAlloc *alloc);

/* Device mirror of a decoder (dictionary interface).  LzmaDec_DecodeToDic /
 * LzmaDec_DecodeToBuf keep the decoder's dictionary, probability table and
 * state on the GPU between calls (keyed by the CLzmaDec address, its dic,
 * dicBufSize and probs allocation, and the current device): a call uploads
 * its input only -- plus, once per mirror, the dictionary history a
 * continuing decoder needs -- and downloads the bytes it decoded, the state
 * and the table.  Bytes of dic the CALLER writes between calls are seen when
 * it moves dicPos / processedPos over them as the reference's LZMA2 walker
 * does (Lzma2Dec.c:159-166: the call uploads exactly that span); any other
 * change of the positions, or of the host table, makes the call start from
 * the host copies.  A caller rewriting bytes it already handed to the decoder
 * without moving the positions is not detected: LzmaGpu_DecoderRelease(p)
 * drops the mirror (as do LzmaDec_FreeProbs / LzmaDec_Free and any change of
 * dic, dicBufSize or probs), so the next call starts from the host copy.  A
 * decoder used on another device drops its mirrors on the others.  Mirrors
 * beyond 256 decoders or 16 GiB (LZGPU_MIRROR_BUDGET_MB) are evicted least
 * recently used first. */
void LzmaGpu_DecoderRelease(const CLzmaDec *p);
/* Host<->device bytes moved by the drop-in decode entry points (LzmaDecode,
 * LzmaUncompress, Lzma2Decode, LzmaDec_DecodeToDic / DecodeToBuf and the LZMA2
 * streaming calls built on them) since start or the last reset, and the number
 * of decode calls that reached the device; reset != 0 zeroes them.  Any
 * argument may be NULL.  Process-wide. */
void LzmaGpu_DropinTransferStats(uint64_t *h2d_bytes, uint64_t *d2h_bytes, uint64_t *calls,
                                 int reset);
/* Coalesced calls (round 4): LzmaDecode / LzmaUncompress / Lzma2Decode calls
 * made by several host threads at once share batch launches, and so do
 * LzmaDec_DecodeToDic / LzmaDec_DecodeToBuf calls on different decoders (one
 * launch of the session kernels, one wave per decoder) -- group commit per
 * device: calls arriving while a launch runs form the next one; a lone
 * caller's launch has one item.  Counts since start or the last reset, summed
 * over devices and both kinds: launches, calls they carried, the largest
 * launch.  LZGPU_COALESCE=0 gives every call its own launch.  Any argument may
 * be NULL. */
void LzmaGpu_CoalesceStats(uint64_t *batches, uint64_t *calls, uint64_t *max_batch, int reset);
/* Host nanoseconds the one-call batches (LzmaDecode, LzmaUncompress,
 * Lzma2Decode) spent per phase, summed over batches since the last reset:
 * ns[0] plan, [1] staging (buffers, packing), [2] upload enqueue, [3] launch
 * enqueue, [4] waiting for the kernel and the results, [5] output download,
 * [6] whole batches, [7] every call from entry to return (queueing included);
 * *batches = batches timed.  Either pointer may be NULL. */
#define LZMA_GPU_COALESCE_PHASES 8
void LzmaGpu_CoalesceTimes(uint64_t *ns, uint64_t *batches, int reset);
/* Which path the drop-in decode entry points took, counted once per batch,
 * call or launch since start or the last reset (the paths are picked by size
 * fields; reading the counts changes nothing): counts[0] one-call batches
 * staged through pinned memory, [1] staged from the callers' pageable buffers,
 * [2] whose outputs were downloaded per call instead of in one transfer;
 * dictionary-interface calls [3] with and [4] without pinned staging, [5]
 * launched on the wave-cooperative and [6] on the one-lane session kernel, [7]
 * session launches that carried both kinds; [8] uploads of a whole dictionary
 * as history; spans written by the host between two calls uploaded in [9] one
 * piece and [10] two pieces (across the ring end); [11] mirrors evicted by
 * count or byte budget; [12] pooled device buffers reused.  counts holds
 * LZMA_GPU_DROPIN_PATHS values and may be NULL (reset only).  Process-wide. */
#define LZMA_GPU_DROPIN_PATHS 13
void LzmaGpu_DropinPathStats(uint64_t *counts, int reset);

/* ---------------------------------------------------------------- drop-in LzmaLib.h */

int LzmaUncompress(unsigned char *dest, size_t *destLen, const unsigned char *src,
                   SizeT *srcLen, const unsigned char *props, size_t propsSize);

/* ---------------------------------------------------------------- drop-in Lzma2Dec.h */

typedef struct {
  CLzmaDec decoder;
  UInt32 packSize;
  UInt32 unpackSize;
  int state;
  Byte control;
  Bool needInitDic;
  Bool needInitState;
  Bool needInitProp;
} CLzma2Dec;

#define Lzma2Dec_Construct(p) LzmaDec_Construct(&(p)->decoder)
#define Lzma2Dec_FreeProbs(p, alloc) LzmaDec_FreeProbs(&(p)->decoder, alloc);
#define Lzma2Dec_Free(p, alloc) LzmaDec_Free(&(p)->decoder, alloc);

SRes Lzma2Dec_AllocateProbs(CLzma2Dec *p, Byte prop, ISzAlloc *alloc);
SRes Lzma2Dec_Allocate(CLzma2Dec *p, Byte prop, ISzAlloc *alloc);
void Lzma2Dec_Init(CLzma2Dec *p);
SRes Lzma2Dec_DecodeToDic(CLzma2Dec *p, SizeT dicLimit, const Byte *src, SizeT *srcLen,
                          ELzmaFinishMode finishMode, ELzmaStatus *status);
SRes Lzma2Dec_DecodeToBuf(CLzma2Dec *p, Byte *dest, SizeT *destLen, const Byte *src,
                          SizeT *srcLen, ELzmaFinishMode finishMode, ELzmaStatus *status);
SRes Lzma2Decode(Byte *dest, SizeT *destLen, const Byte *src, SizeT *srcLen, Byte prop,
                 ELzmaFinishMode finishMode, ELzmaStatus *status, ISzAlloc *alloc);

/* ---------------------------------------------------------------- batch extension */

#define LZMA_GPU_KIND_LZMA 0  /* .lzma-style stream: props[0..5) = 5-byte header */
#define LZMA_GPU_KIND_LZMA2 1 /* LZMA2 byte range: props[0] = dictionary prop byte */
#define LZMA_GPU_NO_WORKSPACE (~(uint64_t)0)

/* One stream of a batch (48 bytes).  Offsets index the caller's packed
 * device buffers. probs_off is filled by LzmaGpu_PlanBatch. */
typedef struct LzmaGpuStreamDesc {
  uint64_t src_off;   /* compressed bytes start in d_src */
  uint64_t src_len;   /* compressed bytes available (*srcLen in) */
  uint64_t dst_off;   /* output window start in d_dst (window == dictionary) */
  uint64_t dst_cap;   /* output capacity (*destLen in) */
  uint64_t probs_off; /* in CLzmaProb cells, into the workspace */
  uint8_t props[5];
  uint8_t props_size;  /* propSize argument of LzmaDecode, normally 5 */
  uint8_t finish_mode; /* ELzmaFinishMode */
  uint8_t kind;        /* LZMA_GPU_KIND_* */
} LzmaGpuStreamDesc;

/* Per-stream outcome (24 bytes): exactly LzmaDecode's return value, *status
 * (-1 where LzmaDecode leaves it untouched), *destLen and *srcLen. */
typedef struct LzmaGpuResult {
  int32_t res;
  int32_t status;
  uint64_t dest_len;
  uint64_t src_len;
} LzmaGpuResult;

/* Host-side planner.  Fills descs[i].probs_off (16-byte aligned slices) and,
 * if order != NULL, a lane->stream permutation that groups streams of equal
 * table width and similar length into the same wavefront.  Returns the
 * workspace size in bytes (0 for n == 0). */
size_t LzmaGpu_PlanBatch(LzmaGpuStreamDesc *descs, size_t n, uint32_t *order);

/* Launch plan for LzmaGpu_DecodeBatchEx (filled by LzmaGpu_PlanBatchEx).
 * The lane order is partitioned: order[0, n_lds) runs on the LDS kernel in
 * n_classes launches by table width (class k: classes[k].n consecutive lanes,
 * per-stream probability tables in LDS, lanes_per_group streams per
 * workgroup); order[n_lds, n) runs on the generic kernel (tables in the
 * global workspace: lc + lp too wide for LDS).  Per-call overrides:
 * LzmaGpu_PlanBatchOpt.  PlanBatchEx reads experiment overrides from the
 * environment on every call: LZGPU_KERNEL=global|throughput|latency|coop,
 * LZGPU_LANES=<streams per workgroup>, LZGPU_GROUPS=<workgroups per CU>,
 * LZGPU_OCC=<1|2|4 waves per SIMD>, LZGPU_CUS, LZGPU_COOP=0|1,
 * LZGPU_PERSIST=0 (one stream per lane), LZGPU_CLASSES=1 (one LDS launch),
 * LZGPU_SLICE_ALIGN8=1, LZGPU_KERNEL_LZMA2=1, LZGPU_COOP_LAT=1, LZGPU_MERGE_LAT=0, LZGPU_ILV=0,
 * LZGPU_ILV_ANY=1, LZGPU_THR_FIT=0 (the
 * LZMA_GPU_PLAN_* flags below); DecodeBatchEx reads LZGPU_CLASS_STREAMS=0
 * (classes launched one after another on the caller's stream).
 * workspace_bytes includes the LDS launches' work counters at queue_offset
 * (zeroed by every DecodeBatchEx launch on its stream). */
#define LZMA_GPU_MAX_CLASSES 4
/* One LDS-kernel launch: `n` consecutive lanes of the order, tables of at most
 * lds_cells_per_lane cells, lanes_per_group streams per workgroup,
 * groups_per_cu workgroups per CU, register budget waves_per_simd. */
typedef struct LzmaGpuLdsClass {
  uint64_t n;
  uint32_t lanes_per_group;
  uint32_t lds_cells_per_lane;
  uint32_t groups_per_cu;
  uint32_t waves_per_simd;
  uint32_t lds_mask;      /* which probability sections live in LDS */
  uint32_t flags;         /* LZMA_GPU_CLASS_*: set by the planner */
  /* lane-interleaved global sections (lds_mask bit 30; the throughput
   * placement's default, LZMA_GPU_PLAN_NO_ILV turns it off): the class's slot
   * area in the workspace, in 16-bit cells -- slot_groups workgroups, each lane
   * group of 32 owning slot_cells rows of 32 cells; its streams get no
   * per-stream slice (probs_off 0) */
  uint64_t slot_off;
  uint32_t slot_cells;
  uint32_t slot_groups;
} LzmaGpuLdsClass;
/* the class holds LZMA2 items: launched on the kernel build with the LZMA2 chunk
 * walker (without it the LZMA-only build runs, fewer registers) */
#define LZMA_GPU_CLASS_HAS_LZMA2 1u

typedef struct LzmaGpuPlan {
  uint64_t workspace_bytes;
  uint64_t n;
  uint64_t n_lds;           /* lanes on the LDS kernel: sum of classes[k].n */
  uint32_t lanes_per_group; /* the class with the most streams (summary) */
  uint32_t lds_cells_per_lane;
  uint32_t groups_per_cu;
  uint32_t waves_per_simd;
  uint64_t queue_offset;    /* class k's work counter at queue_offset + 64 k */
  uint32_t persistent;      /* 1: grid = resident workgroups, lanes pull streams from the queue */
  uint32_t n_classes;       /* LDS launches, by table width (mixed lc/lp/pb batches) */
  LzmaGpuLdsClass classes[LZMA_GPU_MAX_CLASSES];
} LzmaGpuPlan;

SRes LzmaGpu_PlanBatchEx(LzmaGpuStreamDesc *descs, size_t n, uint32_t *order, LzmaGpuPlan *plan);

/* Per-call planner options (LzmaGpu_PlanBatchOpt).  Zero = the planner's own
 * choice for every field; the environment is not read.  `kernel` forces the
 * instantiation every LDS-eligible class runs on:
 *   THROUGHPUT  placement 0x105 (per-symbol tables in LDS), up to 32 streams
 *               per wave -- the config-3 kernel, whatever the batch size;
 *   LATENCY     placement 0x1BF, one stream per wave (lanes_per_group may
 *               widen it);
 *   COOP        one stream per 32-lane wave, every lane holding the
 *               stream's state (match copies and direct distance bits
 *               spread over the lanes); placement 0x7FF (all sections in
 *               LDS) where the whole table fits, else 0x1BF;
 *   GLOBAL      every stream on the generic kernel (tables in global memory).
 * A class whose latency-placement table exceeds the LDS limit keeps the
 * throughput placement.  cus: CUs to size the plan for (0 = the device's). */
#define LZMA_GPU_KERNEL_AUTO 0
#define LZMA_GPU_KERNEL_THROUGHPUT 1
#define LZMA_GPU_KERNEL_LATENCY 2
#define LZMA_GPU_KERNEL_COOP 3
#define LZMA_GPU_KERNEL_GLOBAL 4
typedef struct LzmaGpuPlanOptions {
  uint32_t kernel;          /* LZMA_GPU_KERNEL_* */
  uint32_t cus;             /* 0 = current device's CU count (256 without a device) */
  uint32_t lanes_per_group; /* 0 = planner; else streams per workgroup (<= 64) */
  uint32_t groups_per_cu;   /* 0 = planner */
  uint32_t waves_per_simd;  /* 0 = planner; else register budget 1|2|4 */
  uint32_t persistent;      /* 0 = default (on), 1 = on, 2 = off (one stream per lane) */
  uint32_t coop;            /* AUTO only: 0 = by streams per CU, 1 = always, 2 = never */
  uint32_t one_class;       /* 1: all LDS-eligible streams in one launch */
  uint32_t flags;           /* LZMA_GPU_PLAN_* bits */
  /* reserved, 0 (round 4's scalar-register share of one-lane waves, measured
   * slower at every share and removed in round 5) */
  uint32_t reserved;
} LzmaGpuPlanOptions;
/* per-lane LDS slices 8-byte aligned (default: an odd number of dwords, so that
 * 32 lanes reading the same cell index hit 32 different LDS banks) */
#define LZMA_GPU_PLAN_SLICE_ALIGN8 1u
/* every class on the kernel build with the LZMA2 chunk walker (A/B only) */
#define LZMA_GPU_PLAN_KERNEL_LZMA2 2u
/* cooperative classes keep the latency placement 0x1BF (SpecPos, matched-
 * literal trees and LenHigh in global memory).  Default: every section in LDS
 * (placement 0x7FF) when the whole table fits the class's streams per CU --
 * config 4 2.85 -> 3.00 GB/s, the xz leg 2.52 -> 2.63 (profiles/r02_ab/). */
#define LZMA_GPU_PLAN_COOP_LAT 4u
/* one class per table-width bucket even when several land in the one-lane
 * latency regime (default: those are merged into one class, one launch) */
#define LZMA_GPU_PLAN_NO_MERGE_LAT 8u
/* throughput classes keep the probability sections that are not in LDS in
 * per-stream slices (the round-2 layout) instead of lane-interleaved -- cell i
 * of the 32 lanes of a lane group side by side -- in a slot area per class
 * (LZGPU_ILV=0) */
#define LZMA_GPU_PLAN_NO_ILV 16u
/* A/B: interleaved rows for throughput waves of any width up to 64 lanes, not
 * only whole 32-lane groups (LZGPU_ILV_ANY=1); a class whose 32-lane row of LDS
 * slices would not fit a CU's LDS keeps its per-lane slices */
#define LZMA_GPU_PLAN_ILV_ANY 32u
/* Default: a single-class batch of 17 to 63 streams per CU in the latency
 * regime (a strong-scaling share, e.g. 8,192 x 4 KiB on 256 CUs) runs waves
 * of 2-4 streams so that every stream is resident at once, instead of
 * one-stream waves in several rounds.  This flag restores the round-2 shape
 * (LZGPU_THR_FIT=0). */
#define LZMA_GPU_PLAN_NO_THR_FIT 64u

/* Default: a one-lane latency class with more streams per CU than its widest
 * slice lets resident (lc + lp = 4 at pb = 4 takes 9 of a CU's 128 LDS blocks:
 * 14 workgroups) keeps its slot trees in the global rows instead, 8 blocks and
 * 16 workgroups per CU.  This flag keeps them in LDS (LZGPU_SLOTG=0). */
#define LZMA_GPU_PLAN_NO_SLOTG 256u
/* 128u was LZMA_GPU_PLAN_STEP (round 4's decision-level kernel, removed in
 * round 5): reserved, rejected with SZ_ERROR_PARAM so that a caller built
 * against the old header is told rather than silently given another flag. */
#define LZMA_GPU_PLAN_KNOWN_FLAGS 0x17Fu

/* LzmaGpu_PlanBatchEx with explicit options (opt == NULL: as PlanBatchEx,
 * whose defaults take the LZGPU_* experiment variables of the environment,
 * read per call).  SZ_ERROR_PARAM on an unknown kernel value or a flag bit
 * outside LZMA_GPU_PLAN_KNOWN_FLAGS. */
SRes LzmaGpu_PlanBatchOpt(LzmaGpuStreamDesc *descs, size_t n, uint32_t *order, LzmaGpuPlan *plan,
                          const LzmaGpuPlanOptions *opt);

/* Decode a planned batch (order is required: the plan's lane partition). */
SRes LzmaGpu_DecodeBatchEx(const LzmaGpuPlan *plan, const LzmaGpuStreamDesc *d_descs,
                           const uint32_t *d_order, const Byte *d_src, Byte *d_dst,
                           void *d_workspace, LzmaGpuResult *d_results, void *stream);

/* Decode n streams on the current HIP device (generic kernel, any plan).  All pointers are device
 * memory owned by the caller; d_order may be NULL (identity).  Asynchronous
 * on `stream` (a hipStream_t; NULL = default stream).  Returns SZ_OK if the
 * launch was queued; per-stream outcomes land in d_results. */
SRes LzmaGpu_DecodeBatch(const LzmaGpuStreamDesc *d_descs, const uint32_t *d_order, size_t n,
                         const Byte *d_src, Byte *d_dst, void *d_workspace,
                         size_t workspace_bytes, LzmaGpuResult *d_results, void *stream);

/* Convenience: the same over host buffers (allocates, copies, decodes,
 * copies back, frees).  descs need not be planned. */
SRes LzmaGpu_DecodeBatchHost(const LzmaGpuStreamDesc *descs, size_t n, const Byte *src,
                             size_t src_bytes, Byte *dst, size_t dst_bytes,
                             LzmaGpuResult *results);
/* The same with planner options (NULL = PlanBatchEx defaults); the plan used
 * is returned through plan_out when given. */
SRes LzmaGpu_DecodeBatchHostOpt(const LzmaGpuStreamDesc *descs, size_t n, const Byte *src,
                                size_t src_bytes, Byte *dst, size_t dst_bytes,
                                LzmaGpuResult *results, const LzmaGpuPlanOptions *opt,
                                LzmaGpuPlan *plan_out);

/* Split an LZMA2 stream into its independently decodable blocks: a block
 * starts at every chunk that resets the dictionary (control 0x01 or
 * >= 0xE0, Lzma2Dec.c:14-26) and runs to the next one.  Walks chunk headers
 * only (O(#chunks)).  For block i: src_off/src_len = its byte range
 * (the final EOS byte belongs to no block), unpack = its decoded size.
 * Returns the number of blocks (may exceed max_blocks: then only the first
 * max_blocks are written) or (size_t)-1 on a malformed header sequence. */
size_t Lzma2Gpu_SplitBlocks(const Byte *src, size_t src_len, uint64_t *src_off,
                            uint64_t *block_src_len, uint64_t *unpack, size_t max_blocks);

/* ---------------------------------------------------------------- streaming sessions */

/* A device-resident decoder: the CLzmaDec state (LzmaDec.h:50-69) plus one
 * call's arguments and results.  Many concurrent zlib-like streams (the fork's
 * SzDecodeLzmaToFileWithBuf pattern, 7zDec.c:567-648) advance by one batched
 * launch per round of calls; the state stays in device memory between calls.
 * All pointers are device memory. */
typedef struct LzmaGpuSession {
  uint32_t lc, lp, pb, dict_size;          /* CLzmaProps */
  uint16_t *probs;                         /* LzmaGpu_SessionProbsBytes() bytes */
  Byte *dic;                               /* dictionary (a ring for DecodeToBuf) */
  const Byte *in;                          /* this call: input */
  uint64_t dic_buf_size, dic_pos, dic_limit, in_len, in_used;
  uint32_t range, code, processed_pos, check_dic_size, state;
  uint32_t reps[4];
  uint32_t remain_len, need_flush, need_init_state, temp_buf_size;
  int32_t finish_mode, res, status;        /* this call: finish mode; results */
  int32_t mode;                            /* 0: DecodeToDic(dic_limit), 1: DecodeToBuf */
  Byte temp_buf[LZMA_REQUIRED_INPUT_MAX];
  Byte _pad[4];
  Byte *out;                               /* DecodeToBuf: destination */
  uint64_t out_len;                        /* DecodeToBuf: in = room, out = bytes written */
} LzmaGpuSession;

/* Device bytes a session's probability table needs for these props (0 on bad props). */
size_t LzmaGpu_SessionProbsBytes(const Byte *props, unsigned propsSize);
/* Host-side LzmaDec_Allocate + LzmaDec_Init on a session struct (LzmaDec.c:950-970,
 * 685-705): parses props, binds the caller's device probs / dictionary
 * (dic_buf_size >= 1; LzmaDec_Allocate uses the props' dictionary size). */
SRes LzmaGpu_SessionInit(LzmaGpuSession *s, const Byte *props, unsigned propsSize,
                         uint16_t *d_probs, Byte *d_dic, size_t dic_buf_size);
/* One call per session, all in one launch: for mode 0 exactly
 * LzmaDec_DecodeToDic(s, dic_limit, in, &in_len -> in_used, finish_mode, &status),
 * for mode 1 exactly LzmaDec_DecodeToBuf(s, out, &out_len, in, &in_len -> in_used,
 * finish_mode, &status); res / status / in_used / out_len and the decoder state are
 * written back into each d_sessions[i].  Asynchronous on `stream`. */
SRes LzmaGpu_SessionDecodeBatch(LzmaGpuSession *d_sessions, size_t n, void *stream);

/* ---------------------------------------------------------------- time-sliced batches */

/* A batch of LZMA streams decoded in rounds.  Each round is one launch in
 * which every unfinished stream makes one LzmaDec_DecodeToDic call
 * (LzmaDec.c:719-838) on its device-resident decoder (an LzmaGpuSession in the
 * workspace) with dicLimit = dicPos + slice_bytes and LZMA_FINISH_ANY -- the
 * call that reaches dst_cap takes the stream's own finish mode -- and its
 * state is spilled back for the next round (the CLzmaDec checkpoint,
 * LzmaDec.h:50-69).  Streams that finish drop out; the next round deals the
 * unfinished ones over every CU again.  Results (output bytes and
 * LzmaGpuResult) equal LzmaGpu_DecodeBatchEx's, i.e. LzmaDecode's per stream.
 * A round's launch is bounded by slice_bytes of output per stream, so work of
 * other streams or tenants queued on the device waits at most one round
 * behind a long stream, and a caller can stop after any round and resume --
 * with one exception: a stream whose round hits SZ_ERROR_DATA is decoded
 * again from its start in that same round as one unbounded call (the
 * reference's results on corrupt input depend on where its calls start,
 * LzmaDec.c:797,826; sliced.hip), so one corrupt long stream can hold a round
 * for a whole stream's worth of decode.
 * LZMA items only (an LZMA2 item: SZ_ERROR_PARAM at plan time). */
#define LZMA_GPU_SLICED_AUTO 0u
#define LZMA_GPU_SLICED_LANE 1u   /* one stream per wave, its table staged in LDS per round */
#define LZMA_GPU_SLICED_COOP 2u   /* one stream per 32-lane wave (the wave-cooperative decoder) */
#define LZMA_GPU_SLICED_GLOBAL 3u /* one stream per lane, table in the workspace (any lc/lp) */
typedef struct LzmaGpuSlicedPlan {
  uint64_t workspace_bytes;
  uint64_t n;
  uint64_t slice_bytes;
  uint32_t rounds;          /* launches that take every stream to its end: ceil(max dst_cap / slice) */
  uint32_t kernel;          /* LZMA_GPU_SLICED_* that runs */
  uint32_t table_cells;     /* LDS cells staged per stream (the widest, <= 32768) */
  uint32_t groups_per_cu;   /* resident workgroups per CU (persistent grid) */
  uint32_t max_groups;      /* grid of every round launch */
  uint32_t lds_mask;        /* LANE: sections staged in LDS (0x7FF all; 0x200001BF the
                               latency kernel's, the others used in place) */
  uint64_t sess_off, list_off, ctr_off; /* workspace sections (bytes) */
  uint64_t n_inplace;       /* streams whose table is wider than the staged slot: decoded
                               in place by the global kernel each round */
} LzmaGpuSlicedPlan;
/* Plan a sliced batch: fills descs[i].probs_off (the stream's table, in cells
 * into the workspace, 16-byte aligned), order (if not NULL: longest work
 * first, uploaded by the caller as DecodeBatchSliced's d_order) and *plan.
 * kernel = LZMA_GPU_SLICED_*; AUTO picks COOP for at most 8 streams per CU,
 * else LANE, and GLOBAL when no table fits LDS; streams whose table does not
 * fit the LDS kernel's slot (over 64 KiB) run in place on the global kernel
 * in the same rounds (plan->n_inplace).  SZ_ERROR_PARAM: slice_bytes == 0,
 * an LZMA2 item, more than 2^24 rounds. */
SRes LzmaGpu_PlanSliced(LzmaGpuStreamDesc *descs, size_t n, uint64_t slice_bytes, unsigned kernel,
                        uint32_t *order, LzmaGpuSlicedPlan *plan);
/* Enqueue rounds [first_round, first_round + n_rounds) of a planned batch on
 * `stream` (n_rounds 0 = every remaining round).  first_round 0 also resets
 * the workspace's counters and spills every stream's initial state.  Device
 * pointers as for DecodeBatchEx; d_order may be NULL (identity). */
SRes LzmaGpu_DecodeBatchSliced(const LzmaGpuSlicedPlan *plan, const LzmaGpuStreamDesc *d_descs,
                               const uint32_t *d_order, const Byte *d_src, Byte *d_dst,
                               void *d_workspace, LzmaGpuResult *d_results, unsigned first_round,
                               unsigned n_rounds, void *stream);
/* Streams still unfinished when round `round` starts (round = plan->rounds:
 * after the last; 0 once every stream is done).  Synchronises `stream`. */
SRes LzmaGpu_SlicedActive(const LzmaGpuSlicedPlan *plan, const void *d_workspace, unsigned round,
                          size_t *active, void *stream);
/* Host-buffer form (uploads, every round, downloads); plan_out may be NULL. */
SRes LzmaGpu_DecodeBatchSlicedHost(const LzmaGpuStreamDesc *descs, size_t n, const Byte *src,
                                   size_t src_bytes, Byte *dst, size_t dst_bytes,
                                   LzmaGpuResult *results, uint64_t slice_bytes, unsigned kernel,
                                   LzmaGpuSlicedPlan *plan_out);

/* ---------------------------------------------------------------- CRC-32 */

/* Drop-ins for 7zCrc.h (poly 0xEDB88320, 7zCrc.c:7):
 *   CrcGenerateTable  replaces 7zCrc.h:14 / 7zCrc.c:56-80 (no-op: device tables are constants)
 *   CrcUpdate         replaces 7zCrc.h:20 / 7zCrc.c:44-47 (raw register, no final XOR)
 *   CrcCalc           replaces 7zCrc.h:21 / 7zCrc.c:49-52 (init and final XOR 0xFFFFFFFF)
 * Over host buffers (upload + the batch kernels).  They have no error
 * channel: without a device they print once to stderr and return 0. */
void CrcGenerateTable(void);
UInt32 CrcUpdate(UInt32 crc, const void *data, size_t size);
UInt32 CrcCalc(const void *data, size_t size);

/* Batch CRC: range i is d_data[off[i] .. off[i] + len[i]).  Ranges are cut into
 * 2048-byte chunks (aligned to the range end) that decode in parallel.
 * Plan on the host from per-range capacities (len[i] <= caps[i]):
 *   n_chunks = CrcGpu_PlanChunks(caps, n, NULL, NULL);
 *   CrcGpu_PlanChunks(caps, n, chunk_base, chunk_range);  // n and n_chunks entries
 * then upload chunk_base / chunk_range.  Returns (size_t)-1 if n_chunks
 * would exceed 2^32 - 1.  d_chunk_crc: n_chunks uint32 of device scratch. */
size_t CrcGpu_PlanChunks(const uint64_t *caps, size_t n, uint32_t *chunk_base,
                         uint32_t *chunk_range);
/* d_crc[i] = register after range i from `init`, XOR `xorout`
 * (CrcCalc: init = xorout = 0xFFFFFFFF; CrcUpdate(v, ...): init = v, xorout = 0).
 * All pointers device memory; asynchronous on `stream`. */
SRes CrcGpu_Batch(const Byte *d_data, const uint64_t *d_off, const uint64_t *d_len, size_t n,
                  const uint32_t *d_chunk_base, const uint32_t *d_chunk_range, size_t n_chunks,
                  uint32_t init, uint32_t xorout, uint32_t *d_chunk_crc, uint32_t *d_crc,
                  void *stream);
/* CrcCalc of every decoded stream of a batch, straight from the decode's device
 * buffers: d_crc[i] = CrcCalc(d_dst + descs[i].dst_off, results[i].dest_len)
 * (the 7z folder / file check after decode, 7zIn.c:1380, 1397).  Plan with
 * capacities = descs[i].dst_cap via LzmaGpu_Crc32Plan (host descs). */
size_t LzmaGpu_Crc32Plan(const LzmaGpuStreamDesc *descs, size_t n, uint32_t *chunk_base,
                         uint32_t *chunk_range);
SRes LzmaGpu_Crc32Batch(const LzmaGpuStreamDesc *d_descs, const LzmaGpuResult *d_results,
                        size_t n, const Byte *d_dst, const uint32_t *d_chunk_base,
                        const uint32_t *d_chunk_range, size_t n_chunks, uint32_t *d_chunk_crc,
                        uint32_t *d_crc, void *stream);

/* ---------------------------------------------------------------- xz, x86 BCJ, CRC-64 */

/* x86 BCJ converter, drop-in for Bra.h:58 / Bra86.c:11-85 (x86_Convert: the
 * branch-target filter of 7z and xz; encoding 0 = decode).  Runs on the GPU
 * over the caller's host buffer; returns the bytes processed (the last <= 4
 * are left for the next call), *state carried like the reference's.  No
 * error channel: without a device it prints once and returns 0. */
SizeT x86_Convert(Byte *data, SizeT size, UInt32 ip, UInt32 *state, int encoding);

/* Batch x86 BCJ over device ranges, one lane per range, in place:
 * d_data[off[i] .. off[i] + len[i]) converted with start ip[i] and state
 * d_state[i] (in/out); d_done[i] = bytes processed.  Asynchronous on stream. */
SRes BcjGpu_X86Batch(Byte *d_data, const uint64_t *d_off, const uint64_t *d_len,
                     const uint32_t *d_ip, uint32_t *d_state, uint64_t *d_done, size_t n,
                     int encoding, void *stream);

/* RISC branch converters, drop-ins for Bra.h:59-63 (Bra.c ARM_Convert :6,
 * ARMT_Convert :33, PPC_Convert :68, SPARC_Convert :99; BraIA64.c
 * IA64_Convert :14): the same in-place conversion of the caller's host buffer,
 * computed on the GPU; returns the bytes processed (0 without a device).
 * ARM/PPC/SPARC convert one lane per 4-byte word, IA64 one per 16-byte bundle,
 * ARMT one lane per buffer (its matches chain). */
SizeT ARM_Convert(Byte *data, SizeT size, UInt32 ip, int encoding);
SizeT ARMT_Convert(Byte *data, SizeT size, UInt32 ip, int encoding);
SizeT PPC_Convert(Byte *data, SizeT size, UInt32 ip, int encoding);
SizeT SPARC_Convert(Byte *data, SizeT size, UInt32 ip, int encoding);
SizeT IA64_Convert(Byte *data, SizeT size, UInt32 ip, int encoding);

/* Delta filter, drop-ins for Delta.h:13-15 (Delta.c:6 Delta_Init, :20
 * Delta_Encode, :42 Delta_Decode).  state: DELTA_STATE_SIZE (256) bytes,
 * delta in 1..256; data converted in place on the GPU, state carried. */
#define LZMA_GPU_DELTA_STATE_SIZE 256
void Delta_Init(Byte *state);
void Delta_Encode(Byte *state, unsigned delta, Byte *data, SizeT size);
void Delta_Decode(Byte *state, unsigned delta, Byte *data, SizeT size);

/* Batch forms over device ranges, in place, asynchronous on stream.
 * BraGpu_Batch: kind = the xz filter ID (5 PPC, 6 IA64, 7 ARM, 8 ARMT,
 * 9 SPARC; else SZ_ERROR_UNSUPPORTED); range i starts at ip[i];
 * d_done[i] = what the reference's Convert returns for it.
 * DeltaGpu_Batch: d_delta[i] in 1..256 (unchecked on the device), d_state:
 * n x 256 bytes, range i's state at d_state + 256 * i (in/out). */
SRes BraGpu_Batch(unsigned kind, Byte *d_data, const uint64_t *d_off, const uint64_t *d_len,
                  const uint32_t *d_ip, uint64_t *d_done, size_t n, int encoding, void *stream);
SRes DeltaGpu_Batch(Byte *d_data, const uint64_t *d_off, const uint64_t *d_len,
                    const uint32_t *d_delta, Byte *d_state, size_t n, int encoding, void *stream);

/* BCJ2 (Bcj2.c:28-128), the four-stream x86 branch decoder of 7z: buf0 = main
 * stream, buf1 = CALL targets, buf2 = JMP / Jcc targets, buf3 = the range-coded
 * "converted" bits.  Bcj2_Decode replaces Bcj2.h:54-59 (host buffers, computed
 * on the GPU; buf0 may overlap outBuf as Bcj2.h:36-39 allows): SZ_OK or
 * SZ_ERROR_DATA as the reference, SZ_ERROR_FAIL without a device.
 * Bcj2Gpu_Batch: one lane per job, all pointers device memory, d_res[i] = the
 * SRes of job i; asynchronous on `stream`. */
typedef struct Bcj2GpuJob {   /* 80 bytes */
  const Byte *buf0, *buf1, *buf2, *buf3;
  uint64_t size0, size1, size2, size3;
  Byte *out;
  uint64_t out_size;
} Bcj2GpuJob;
int Bcj2_Decode(const Byte *buf0, SizeT size0, const Byte *buf1, SizeT size1, const Byte *buf2,
                SizeT size2, const Byte *buf3, SizeT size3, Byte *outBuf, SizeT outSize);
SRes Bcj2Gpu_Batch(const Bcj2GpuJob *d_jobs, size_t n, int32_t *d_res, void *stream);

/* The BCJ2 encoder (the reference ships none; csrc/bcj2enc_device.h states the
 * rule): stream i's src_len bytes split into the four streams that Bcj2_Decode
 * merges -- out[0] main, out[1] CALL targets, out[2] JMP / Jcc targets, out[3]
 * the range-coded bits -- a branch being converted when its absolute target
 * lies inside the stream's own bytes.  The split is computed in parallel over
 * positions (a large stream spreads over the chip, small streams share
 * workgroups); only the range coder is one lane per stream, one step per branch
 * opcode.  Per stream:
 *   SZ_OK                 len[k] bytes written at out[k].off
 *   SZ_ERROR_OUTPUT_EOF   a stream outgrew its cap: len[] holds the four true
 *                         lengths; nothing is written at or past a cap (a
 *                         target is written whole or not at all)
 *   SZ_ERROR_UNSUPPORTED  src_len >= 2^31; nothing read or written
 * Bcj2EncGpu_Bound: capacities that hold whatever the data (n, 4 (n / 5),
 * 4 (n / 5), 5 + n). */
typedef struct Bcj2GpuEncRange {
  uint64_t off, cap;          /* in d_dst */
} Bcj2GpuEncRange;
typedef struct Bcj2GpuEncDesc {   /* 80 bytes */
  uint64_t src_off, src_len;  /* in d_src; any byte alignment */
  Bcj2GpuEncRange out[4];     /* main, call, jump, rc */
} Bcj2GpuEncDesc;
typedef struct Bcj2GpuEncResult { /* 40 bytes */
  int32_t res;
  uint32_t _pad;
  uint64_t len[4];            /* main, call, jump, rc */
} Bcj2GpuEncResult;
#define LZMA_GPU_BCJ2_MAIN 0
#define LZMA_GPU_BCJ2_CALL 1
#define LZMA_GPU_BCJ2_JUMP 2
#define LZMA_GPU_BCJ2_RC 3
/* Host only. */
void Bcj2EncGpu_Bound(uint64_t src_len, uint64_t bound[4]);
/* Host only: the bytes of scratch a batch of these descriptors needs (a fixed
 * part plus a slice per stream of about 2 src_len); 16-byte aligned memory. */
uint64_t Bcj2EncGpu_Scratch(const Bcj2GpuEncDesc *descs, size_t n);
/* All pointers device memory, the scratch uninitialised; asynchronous on
 * `stream`; n == 0 is a no-op.  SZ_OK if the launches were queued
 * (SZ_ERROR_PARAM for n above 2^31 - 1, SZ_ERROR_FAIL without a device);
 * per-stream outcomes land in d_results. */
SRes Bcj2EncGpu_EncodeBatch(const Bcj2GpuEncDesc *d_descs, size_t n, const Byte *d_src,
                            Byte *d_dst, void *d_scratch, Bcj2GpuEncResult *d_results,
                            void *stream);
/* The same over host buffers, in as many launches as keep the scratch at or
 * under workspace_limit bytes (0 = half of the device's free memory).
 * SZ_ERROR_MEM if one stream's scratch alone exceeds the limit or an allocation
 * fails, SZ_ERROR_PARAM for a range outside src / dst, SZ_ERROR_FAIL without a
 * device. */
SRes Bcj2EncGpu_EncodeBatchHost(const Bcj2GpuEncDesc *descs, size_t n, const Byte *src,
                                size_t src_size, Byte *dst, size_t dst_size,
                                Bcj2GpuEncResult *results, uint64_t workspace_limit);

/* CRC-64 (XzCrc64.c, poly 0xC96C5795D7870F42).  Crc64Calc drop-in replaces
 * XzCrc64.h:20 / XzCrc64.c:30 (host buffer, GPU compute; 0 without a device).
 * The batch form mirrors CrcGpu_Batch with 2048-byte chunks planned by
 * CrcGpu_PlanChunks; d_chunk_crc: n_chunks uint64 of scratch. */
UInt64 Crc64Calc(const void *data, size_t size);
SRes Crc64Gpu_Batch(const Byte *d_data, const uint64_t *d_off, const uint64_t *d_len, size_t n,
                    const uint32_t *d_chunk_base, const uint32_t *d_chunk_range, size_t n_chunks,
                    uint64_t init, uint64_t xorout, uint64_t *d_chunk_crc, uint64_t *d_crc,
                    void *stream);

/* SHA-256 (FIPS 180-4), drop-ins for Sha256.h:11-22 (Sha256.c:12-204).  CSha256
 * has the reference's layout (104 bytes); after every call state, count and
 * buffer[0 .. count & 63) hold what the reference's hold (Sha256_Final
 * re-initialises the struct).  Every compression runs on the GPU:
 * Sha256_Update uploads the buffered bytes plus the whole 64-byte blocks its
 * data completes and continues from p->state; a call that completes no block
 * only buffers (no device call); Sha256_Final sends the padded tail.  No error
 * channel: without a device the calls print once, the state is left as it is
 * and Sha256_Final writes a zero digest. */
#define SHA256_DIGEST_SIZE 32
typedef struct {
  UInt32 state[8];
  UInt64 count;
  Byte buffer[64];
} CSha256;
void Sha256_Init(CSha256 *p);
void Sha256_Update(CSha256 *p, const Byte *data, size_t size);
void Sha256_Final(CSha256 *p, Byte *digest);

/* Batch form over device ranges: d_digest[32 * i .. + 32) = SHA-256 of
 * d_data[off[i] .. off[i] + len[i]), any byte alignment, any length (0 too).
 * kernel: LANE = one lane per range (many ranges), WAVE = one wave per range
 * (few long ranges: the 64 lanes compute the message schedules of 64
 * consecutive blocks side by side), AUTO = by n alone, the wave kernel up to
 * 1,024 ranges (one per SIMD of the chip) and the lane kernel beyond.  All
 * pointers device memory; asynchronous on `stream`; n == 0 is a no-op.  SZ_ERROR_PARAM: an unknown kernel or n above 2^32 - 1;
 * SZ_ERROR_FAIL without a device. */
#define LZMA_GPU_SHA256_AUTO 0
#define LZMA_GPU_SHA256_LANE 1
#define LZMA_GPU_SHA256_WAVE 2
SRes Sha256Gpu_Batch(const Byte *d_data, const uint64_t *d_off, const uint64_t *d_len,
                     size_t n, unsigned kernel, Byte *d_digest /* n x 32 */, void *stream);

/* xz files as block batches.  The reference decodes xz strictly in order
 * (XzUnpacker_Code, XzDec.c:604-870); the blocks of a multi-block file (and
 * the streams of a concatenated one) are independent, so here the whole file
 * is indexed first -- from each stream's footer and index backwards, as
 * Xzs_ReadBackward does (XzIn.c:150-280) -- and every block decodes as one
 * lane of an LZMA2 batch, then its filter chain (x86 / PPC / IA64 / ARM /
 * ARMT / SPARC branch converters, delta; last filter first, one batch per
 * kind and depth), then the block checks on the GPU (CRC-32, CRC-64 and
 * SHA-256, one batch each over the decode's own buffers; the host only
 * compares the results with the stored check fields). */
#define LZMA_GPU_XZ_CHECK_NONE 0
#define LZMA_GPU_XZ_CHECK_CRC32 1
#define LZMA_GPU_XZ_CHECK_CRC64 4
#define LZMA_GPU_XZ_CHECK_SHA256 10
typedef struct {
  uint64_t header_off;  /* block header, offset in the file */
  uint64_t data_off;    /* first byte of the block's LZMA2 data */
  uint64_t pack_size;   /* LZMA2 data bytes (index unpadded size - header - check) */
  uint64_t unpack_size; /* uncompressed bytes (index) */
  uint64_t dst_off;     /* offset of the block's output in the whole file's output */
  uint64_t check_off;   /* stored check field, offset in the file */
  uint32_t check_type;  /* LZMA_GPU_XZ_CHECK_* of its stream */
  uint32_t check_size;  /* 0, 4, 8 or 32 bytes */
  uint32_t lzma2_prop;  /* dictionary byte of the LZMA2 filter (XZ_ID_LZMA2 0x21) */
  uint32_t x86;         /* 1: an x86 BCJ filter (XZ_ID_X86 4) precedes LZMA2 */
  uint32_t x86_ip;      /* its start offset (4-byte filter props, else 0) */
  uint32_t stream;      /* index of its xz stream in the file */
  uint32_t num_filters; /* filters before LZMA2 (0..3), in header order */
  uint32_t filter_id[3];   /* XZ_ID_Delta 3, X86 4, PPC 5, IA64 6, ARM 7, ARMT 8, SPARC 9 */
  uint32_t filter_prop[3]; /* start offset (branch converters) or distance 1..256 (delta) */
} LzmaGpuXzBlock;

/* Index an xz file (one or more concatenated streams with stream padding).
 * Fills up to `cap` blocks in file order, *n_blocks = the file's block count,
 * *unpack_total = the sum of their sizes.  Header, block-header, index and
 * footer validation follows XzDec.c / XzIn.c: SZ_ERROR_NO_ARCHIVE (magic or
 * stream-header CRC), SZ_ERROR_ARCHIVE (block header or index malformed),
 * SZ_ERROR_CRC (index CRC, index vs footer), SZ_ERROR_UNSUPPORTED (a filter
 * chain other than [x86 BCJ] + LZMA2, or stream flags beyond the check
 * field).  Host only: works without a device. */
SRes LzmaGpu_XzIndex(const Byte *file, size_t size, LzmaGpuXzBlock *blocks, size_t cap,
                     size_t *n_blocks, uint64_t *unpack_total);

/* Decode a whole xz file held in host memory: index, upload, one batch launch
 * over all blocks, BCJ, checks, download.  *destLen in: capacity, out: bytes
 * written (the whole output, or 0 on error).  Returns SZ_OK, an index error
 * above, SZ_ERROR_OUTPUT_EOF (capacity short), SZ_ERROR_DATA (a block's LZMA2
 * data does not decode to exactly its indexed size, ending with the end mark
 * in exactly its indexed bytes) or SZ_ERROR_CRC (a block check or non-zero
 * block padding).  *bad_block = the first failing block, or -1. */
SRes LzmaGpu_XzDecode(Byte *dest, SizeT *destLen, const Byte *file, size_t size,
                      int64_t *bad_block);

/* ---------------------------------------------------------------- PPMd7 (PPMdH) batches */

/* Ppmd7.c + Ppmd7Dec.c on the GPU: the reference's model, sub-allocator and 7z
 * range decoder, one stream per wave, many independent streams per launch.
 * Per stream the outcome is SzDecodePpmd's (7zDec.c:66-122) over a memory
 * buffer of exactly src_len bytes, checked in this order:
 *   order outside 2..64 or mem_size outside 1<<11 .. 0xFFFFFFFF-36
 *                                  SZ_ERROR_UNSUPPORTED, nothing read or written
 *   first byte non-zero, or Code == 0xFFFFFFFF after the 5 init bytes
 *                                  SZ_ERROR_DATA
 *   a read past src_len (it returns 0 and sets the reference's `extra` flag,
 *   tested after the init bytes and after each symbol)   SZ_ERROR_DATA
 *   a negative symbol              SZ_ERROR_DATA
 *   after dst_len symbols: bytes consumed != src_len, or Code != 0
 *                                  SZ_ERROR_DATA
 *   else                           SZ_OK
 * dest_len = symbols written before the loop stopped, src_len = bytes consumed
 * (at most the descriptor's).  Bytes of d_dst outside
 * [dst_off, dst_off + dest_len) are not written. */
#define LZMA_GPU_PPMD7_PROPS_SIZE 5  /* order byte, memSize LE32: the 7z coder props */

/* One stream of a batch (48 bytes).  Offsets index the caller's packed device
 * buffers; any byte alignment for src_off / dst_off.  ws_off: the stream's own
 * slice of the workspace, Ppmd7Gpu_WorkspaceBytes(mem_size) bytes at a multiple
 * of 256 (slices must not overlap; their contents need no initialisation). */
typedef struct Ppmd7GpuStreamDesc {
  uint64_t src_off;   /* packed bytes start in d_src */
  uint64_t src_len;   /* packed bytes (inSize) */
  uint64_t dst_off;   /* output start in d_dst */
  uint64_t dst_len;   /* symbols to decode (outSize) */
  uint64_t ws_off;    /* slice start in d_workspace, bytes */
  uint32_t mem_size;  /* props[1..5), little endian */
  uint32_t order;     /* props[0] */
} Ppmd7GpuStreamDesc;

/* Per-stream outcome (24 bytes). */
typedef struct Ppmd7GpuResult {
  int32_t res;
  uint32_t _pad;
  uint64_t dest_len;
  uint64_t src_len;
} Ppmd7GpuResult;

/* One stream's workspace slice in bytes, a multiple of 256: the model
 * (mem_size plus the reference's alignment offset and list head) and its
 * BinSumm table.  0 for a mem_size outside the range above. */
uint64_t Ppmd7Gpu_WorkspaceBytes(uint32_t mem_size);
/* Decode n streams on the current device, one workgroup of one wave each, in
 * index order (put long streams first).  All pointers are device memory owned
 * by the caller; asynchronous on `stream`; n == 0 is a no-op.  Returns SZ_OK
 * if the launch was queued (SZ_ERROR_FAIL without a device, SZ_ERROR_PARAM for
 * n above 2^31 - 1); per-stream outcomes land in d_results. */
SRes Ppmd7Gpu_DecodeBatch(const Ppmd7GpuStreamDesc *d_descs, size_t n, const Byte *d_src,
                          Byte *d_dst, void *d_workspace, Ppmd7GpuResult *d_results, void *stream);
/* The same over host buffers: stages src and dst, lays the slices out itself
 * (descs[i].ws_off is ignored), orders the streams longest first and decodes in
 * as many launches as keep the workspace at or under workspace_limit bytes
 * (0 = half of the device's free memory).  SZ_ERROR_MEM if one stream's slice
 * alone exceeds the limit or an allocation fails, SZ_ERROR_PARAM for a range
 * outside src / dst, SZ_ERROR_FAIL without a device. */
SRes Ppmd7Gpu_DecodeBatchHost(const Ppmd7GpuStreamDesc *descs, size_t n, const Byte *src,
                              size_t src_size, Byte *dst, size_t dst_size,
                              Ppmd7GpuResult *results, uint64_t workspace_limit);

/* Ppmd7.c + Ppmd7Enc.c on the GPU: the same model behind the reference's 7z
 * range encoder, Ppmd7z_RangeEnc_Init, Ppmd7_EncodeSymbol for each of src_len
 * bytes and Ppmd7z_RangeEnc_FlushData, bit for bit the reference's stream.  No
 * end mark is written (7z streams carry none); src_len == 0 gives the five
 * zero bytes of the flush.  Per stream, checked in this order:
 *   order outside 2..64 or mem_size outside 1<<11 .. 0xFFFFFFFF-36
 *                        SZ_ERROR_PARAM, dest_len = packed_len = 0, nothing
 *                        read or written
 *   stream longer than dst_cap
 *                        SZ_ERROR_OUTPUT_EOF, dest_len == dst_cap, dst holds
 *                        the first dst_cap bytes of the stream and packed_len
 *                        its whole length (the encode runs to the end, so a
 *                        caller can retry with that capacity)
 *   else                 SZ_OK, dest_len == packed_len
 * (SZ_ERROR_FAIL, the stream stopping where it is, if a suffix chain of the
 * model ends without the symbol: the root context holds all 256 bytes, so
 * this does not happen with a slice that nothing else writes.)
 * Bytes of d_dst outside [dst_off, dst_off + dest_len) are never written.
 * PPMd7 has no tight output bound: incompressible input grows, e.g. 4,096
 * random bytes pack to 4,405 at order 2.  Size dst_cap generously and retry
 * the streams that report SZ_ERROR_OUTPUT_EOF with their packed_len. */
typedef struct Ppmd7GpuEncDesc {   /* 48 bytes */
  uint64_t src_off;   /* plain bytes start in d_src */
  uint64_t src_len;   /* plain bytes */
  uint64_t dst_off;   /* packed range start in d_dst */
  uint64_t dst_cap;   /* packed range capacity */
  uint64_t ws_off;    /* slice, Ppmd7Gpu_WorkspaceBytes(mem_size), multiple of 256 */
  uint32_t mem_size;
  uint32_t order;
} Ppmd7GpuEncDesc;

typedef struct Ppmd7GpuEncResult { /* 24 bytes */
  int32_t res;
  uint32_t _pad;
  uint64_t dest_len;    /* bytes written, <= dst_cap */
  uint64_t packed_len;  /* length of the whole stream */
} Ppmd7GpuEncResult;

/* Encode n streams on the current device, one workgroup of one wave each, in
 * index order (put long streams first); slices as for decoding.  All pointers
 * are device memory owned by the caller; asynchronous on `stream`; n == 0 is a
 * no-op.  Returns SZ_OK if the launch was queued (SZ_ERROR_FAIL without a
 * device, SZ_ERROR_PARAM for n above 2^31 - 1); per-stream outcomes land in
 * d_results. */
SRes Ppmd7Gpu_EncodeBatch(const Ppmd7GpuEncDesc *d_descs, size_t n, const Byte *d_src, Byte *d_dst,
                          void *d_workspace, Ppmd7GpuEncResult *d_results, void *stream);
/* The same over host buffers: stages src and dst, lays the slices out itself
 * (descs[i].ws_off is ignored), orders the streams longest src_len first and
 * encodes in as many launches as keep the workspace at or under
 * workspace_limit bytes (0 = half of the device's free memory).  SZ_ERROR_MEM
 * if one stream's slice alone exceeds the limit or an allocation fails,
 * SZ_ERROR_PARAM for a range outside src / dst, SZ_ERROR_FAIL without a
 * device. */
SRes Ppmd7Gpu_EncodeBatchHost(const Ppmd7GpuEncDesc *descs, size_t n, const Byte *src, size_t src_size,
                              Byte *dst, size_t dst_size, Ppmd7GpuEncResult *results,
                              uint64_t workspace_limit);

/* ---------------------------------------------------------------- LZMA encoding */

/* The reference's encoder, one stream per lane, many independent streams per
 * launch (csrc/lzmaenc_device.h).  Mode 0 is what props that normalise to
 * algo == 0 and btMode == 0 select (LzmaEncProps_Normalize, LzmaEnc.c:53-74:
 * levels 0..4): the Hc4 hash-chain finder, GetOptimumFast and the range coder.
 * The normal modes -- the optimal parser (GetOptimum, algo == 1) and / or the
 * binary-tree finder Bt4 (btMode == 1 with numHashBytes 4), what levels 5..9
 * select -- run in a kernel of their own and are opt-in (LzmaEncGpu_SetModes
 * below): they take a larger workspace slice and far longer per byte.  In every
 * mode the bytes are those of the reference's single-threaded LzmaEncode
 * (a build with _7ZIP_ST); nothing is claimed about its multi-threaded match
 * finder, and numThreads is ignored.  Per stream the
 * outcome is LzmaEncode's over a buffer of dst_cap bytes:
 *   SZ_OK                 dest_len bytes written
 *   SZ_ERROR_OUTPUT_EOF   the stream is longer than dst_cap: dest_len == dst_cap
 *                         and dst holds the first dst_cap bytes of the stream
 *   SZ_ERROR_PARAM        lc > 8, lp > 4, pb > 4, dict_size 0 or above 1 << 30,
 *                         fb outside 5..273, mode above 3, or ws_off not a
 *                         multiple of 16; nothing read or written, and the
 *                         stream takes no workspace slice
 *   SZ_ERROR_UNSUPPORTED  src_len >= 2^31; nothing read or written
 * Bytes of d_dst outside [dst_off, dst_off + dest_len) are not written and
 * bytes of d_src outside [src_off, src_off + src_len) are not read. */

#ifndef __LZMA_ENC_H
typedef struct _CLzmaEncProps {   /* 48 bytes, LzmaEnc.h:15-31 */
  int level;
  UInt32 dictSize;
  int lc, lp, pb, algo, fb, btMode, numHashBytes;
  UInt32 mc;
  unsigned writeEndMark;
  int numThreads;
} CLzmaEncProps;
#endif
#ifndef __7Z_TYPES_H
typedef struct {
  SRes (*Progress)(void *p, UInt64 inSize, UInt64 outSize);
} ICompressProgress;
#endif

void LzmaEncProps_Init(CLzmaEncProps *p);
void LzmaEncProps_Normalize(CLzmaEncProps *p);
UInt32 LzmaEncProps_GetDictSize(const CLzmaEncProps *props2);

/* One stream of an encode batch (72 bytes).  Offsets index the caller's packed
 * device buffers; any byte alignment for src_off / dst_off.  The props fields
 * are the normalised ones LzmaEncGpu_DescFromProps writes. */
typedef struct LzmaEncGpuStreamDesc {
  uint64_t src_off;   /* plain bytes start in d_src */
  uint64_t src_len;   /* plain bytes */
  uint64_t dst_off;   /* output start in d_dst */
  uint64_t dst_cap;   /* room for the output */
  uint64_t ws_off;    /* slice start in d_workspace, bytes (LzmaEncGpu_PlanBatch) */
  uint32_t dict_size;
  uint32_t lc, lp, pb;
  uint32_t fb;        /* numFastBytes, 5..273 */
  uint32_t mc;        /* the hash chain's cut value */
  uint32_t write_end_mark;
  uint32_t mode;      /* LZMA_ENC_GPU_MODE_* bits; 0 = the fast path */
} LzmaEncGpuStreamDesc;

#define LZMA_ENC_GPU_MODE_OPTIMAL 1u  /* GetOptimum: algo == 1 */
#define LZMA_ENC_GPU_MODE_BT4 2u      /* Bt4: btMode == 1, numHashBytes 4 */

/* Per-stream outcome (16 bytes). */
typedef struct LzmaEncGpuResult {
  int32_t res;
  uint32_t _pad;
  uint64_t dest_len;
} LzmaEncGpuResult;

#define LZMA_ENC_GPU_LANES_DEFAULT 0u  /* streams per wave: the library's choice */

/* Host only, no device needed.  Normalises *props and applies LzmaEnc_SetProps'
 * checks and clamps (LzmaEnc.c:391-443): SZ_ERROR_PARAM as there; then
 * SZ_ERROR_UNSUPPORTED when the normalised props have algo != 0 or btMode != 0
 * (LzmaGpu_LastError() says so).  On SZ_OK the props fields of *desc are set
 * (its offsets and lengths are left alone) and props5 holds
 * LzmaEnc_WriteProperties' 5 bytes (:2191-2218; the dictionary size is rounded
 * up in the header only).  On an error neither is written. */
SRes LzmaEncGpu_DescFromProps(const CLzmaEncProps *props, int writeEndMark,
                              LzmaEncGpuStreamDesc *desc, Byte props5[5]);
/* The modes the calls that take props may select.  A process-wide atomic mask
 * of LZMA_ENC_GPU_MODE_* bits; its initial value is 0, or the decimal value of
 * the environment variable LZGPU_ENC_MODES, read once.  With the mask at 0
 * every call behaves as described for the fast path alone.  It governs
 * LzmaEncGpu_DescFromProps, Lzma2EncGpu_DescFromProps, LzmaEncode,
 * LzmaCompress, Lzma2Enc_Encode, LzmaGpu_Lzma2EncodeHost, LzmaGpu_XzEncode(Ex),
 * Lzma86_Encode, the Lzma86Gpu_Encode* calls and
 * the LZMA / LZMA2 / BCJ2 folders of LzmaGpu_7zWritePlan and LzmaGpu_7zWrite.
 * SetModes returns the previous mask (bits above 3 are dropped). */
unsigned LzmaEncGpu_SetModes(unsigned allowed);
unsigned LzmaEncGpu_GetModes(void);
/* LzmaEncGpu_DescFromProps with the mask given by the caller: algo == 1 passes
 * when `allowed` has LZMA_ENC_GPU_MODE_OPTIMAL, btMode == 1 when it has
 * LZMA_ENC_GPU_MODE_BT4 and numHashBytes normalises to 4 (Bt2 and Bt3 are
 * SZ_ERROR_UNSUPPORTED whatever the mask).  desc->mode receives the modes the
 * props select.  LzmaGpu_LastError() names the props field that was refused. */
SRes LzmaEncGpu_DescFromPropsEx(const CLzmaEncProps *props, int writeEndMark, unsigned allowed,
                                LzmaEncGpuStreamDesc *desc, Byte props5[5]);
/* Host only.  Lays the workspace out: descs[i].ws_off = start of stream i's
 * slice (probability cells, the `matches` array, the hash, the `son` ring sized
 * by min(dict_size, src_len) + 1 -- twice that with Bt4 -- and, with the
 * optimal parser, the price tables (up to 38 KiB) and the 4,096 `opt` cells
 * (192 KiB); a multiple of 256 bytes; a stream the kernel rejects takes none)
 * and *workspace_bytes = their sum.  The hash is sized by dict_size, not by the
 * source (the reference's hash mask comes from the dictionary, so a smaller one
 * would change the output): level 5's default dictionary of 16 MiB costs about
 * 32 MiB per stream however short the stream, so callers with many small
 * streams should set dictSize.  order (n entries, may be NULL) receives the
 * stream indices grouped by mode -- optimal parser with Bt4, optimal parser
 * with Hc4, Bt4 with the fast parser, then mode 0 -- and within a mode longest
 * source first: the order the lanes should take them in (with every stream at
 * mode 0, longest source first).  SZ_ERROR_PARAM for n above 2^31 - 1. */
SRes LzmaEncGpu_PlanBatch(LzmaEncGpuStreamDesc *descs, size_t n, uint32_t *order,
                          uint64_t *workspace_bytes);
/* Encode n streams on the current device.  All pointers are device memory
 * owned by the caller; d_order (n indices, e.g. LzmaEncGpu_PlanBatch's) may be
 * NULL for index order; the workspace needs no initialisation (the call clears
 * the hashes and sets the probability cells with the whole grid before the
 * encode kernels: one for mode 0 and one for the normal modes, each walking
 * the same order; a lane whose stream belongs to the other returns at once).
 * lanes: streams per 64-lane wave, 64, 32, 16 or LZMA_ENC_GPU_LANES_DEFAULT
 * (the library's choice per kernel).  Asynchronous on `stream`; n == 0 is a no-op.
 * Returns SZ_OK if the launches were queued (SZ_ERROR_FAIL without a device,
 * SZ_ERROR_PARAM for n above 2^31 - 1 or an unknown lanes value); per-stream
 * outcomes land in d_results[i] for stream i. */
SRes LzmaEncGpu_EncodeBatch(const LzmaEncGpuStreamDesc *d_descs, const uint32_t *d_order, size_t n,
                            const Byte *d_src, Byte *d_dst, void *d_workspace,
                            LzmaEncGpuResult *d_results, unsigned lanes, void *stream);
/* The same over host buffers: stages src and dst, plans (descs[i].ws_off is
 * ignored), orders the streams longest first and encodes in as many launches
 * as keep the workspace at or under workspace_limit bytes (0 = half of the
 * device's free memory).  SZ_ERROR_MEM if one stream's slice alone exceeds the
 * limit or an allocation fails, SZ_ERROR_PARAM for a range outside src / dst,
 * SZ_ERROR_FAIL without a device. */
SRes LzmaEncGpu_EncodeBatchHost(const LzmaEncGpuStreamDesc *descs, size_t n, const Byte *src,
                                size_t src_size, Byte *dst, size_t dst_size,
                                LzmaEncGpuResult *results, uint64_t workspace_limit);

/* LzmaEnc.h:72-74 and LzmaLib.h:98-107 as one-item calls of the host form
 * (differences: the drop-in table at the top).  A *propsSize below 5 returns
 * SZ_ERROR_PARAM as the reference does; *destLen is written except on
 * SZ_ERROR_PARAM / SZ_ERROR_UNSUPPORTED / SZ_ERROR_FAIL. */
SRes LzmaEncode(Byte *dest, SizeT *destLen, const Byte *src, SizeT srcLen,
                const CLzmaEncProps *props, Byte *propsEncoded, SizeT *propsSize, int writeEndMark,
                ICompressProgress *progress, ISzAlloc *alloc, ISzAlloc *allocBig);
int LzmaCompress(unsigned char *dest, size_t *destLen, const unsigned char *src, size_t srcLen,
                 unsigned char *outProps, size_t *outPropsSize, int level, unsigned dictSize,
                 int lc, int lp, int pb, int fb, int numThreads);

/* ---------------------------------------------------------------- LZMA encoder sessions */

/* A device-resident fast-mode encoder that takes its stream in pieces: the
 * encoder's counterpart of LzmaGpuSession.  The caller appends plain bytes to
 * src, raises src_len and advances every session of a batch by one round of
 * launches (LzmaEncGpu_SessionEncodeBatch).  After the call with finish == 1,
 * dst[0, out_pos), res and out_pos are LzmaEncode's dest, result and *destLen
 * over the whole input and a buffer of dst_cap bytes, whatever the piece sizes
 * were.  Mode 0 only (levels 0..4: algo 0, btMode 0).
 *
 * Per call the caller sets src_len (bytes of src valid so far; never lower than
 * before, at most src_cap), finish and in_budget, and reads res, status, in_pos
 * and out_pos.  src is append-only and contiguous for the session's life: bytes
 * below src_len stay where they are (the buffer may move between rounds if its
 * content moves with it).  dst[prev out_pos, out_pos) are the call's new bytes;
 * bytes below out_pos are final.
 *
 * A call that is not the last starts a token only while at least
 * LZMA_ENC_GPU_SESSION_HOLD supplied bytes lie ahead of it (every
 * "bytes left" the one-shot encoder looks at is then at its clamp).  So after a
 * call with finish == 0 that ended with status NEEDS_INPUT,
 * src_len - in_pos < LZMA_ENC_GPU_SESSION_HOLD, and a stream shorter than the
 * hold emits nothing before its final call.
 *   status NEEDS_INPUT  everything the hold allows is encoded
 *          BUDGET       in_budget was reached: work is left, call again
 *          FINISHED     the stream is complete (res SZ_OK), did not fit (res
 *                       SZ_ERROR_OUTPUT_EOF: out_pos == dst_cap, dst holds the
 *                       first dst_cap bytes of the full stream) or the record
 *                       was refused (SZ_ERROR_PARAM / SZ_ERROR_UNSUPPORTED:
 *                       props, src_cap >= 2^31, src_len above src_cap or below
 *                       in_pos, ws not 16-byte aligned).  Later calls change
 *                       nothing.
 * in_budget: the call ends at the encoder's first 32 KiB progress step at or
 * after that many input bytes (0 = no bound), which bounds a round's launch. */
#define LZMA_ENC_GPU_SESSION_HOLD 546u   /* 2 * LZMA_MATCH_LEN_MAX */
#define LZMA_ENC_GPU_SESSION_NEEDS_INPUT 0
#define LZMA_ENC_GPU_SESSION_FINISHED 1
#define LZMA_ENC_GPU_SESSION_BUDGET 2

typedef struct LzmaEncGpuSession {   /* 200 bytes */
  const Byte *src;       /* device: the plain stream so far */
  Byte *dst;             /* device: the output */
  void *ws;              /* device: LzmaEncGpu_SessionWorkspaceBytes() bytes, 16-byte aligned */
  uint64_t src_cap;      /* room of src, below 2^31 */
  uint64_t dst_cap;      /* room of dst */
  uint64_t src_len;      /* this call: bytes of src valid so far */
  uint64_t in_budget;    /* this call: input bytes to encode at most; 0 = no bound */
  uint64_t in_pos;       /* result: input bytes encoded so far */
  uint64_t out_pos;      /* result: final bytes in dst */
  uint32_t dict_size, lc, lp, pb, fb, mc, write_end_mark;   /* normalised props */
  uint32_t finish;       /* this call: src_len is the whole stream */
  int32_t res, status;   /* results */
  /* the encoder between calls: set by LzmaEncGpu_SessionInit, then the device's */
  uint32_t needs_init, finished, overflow;
  uint32_t off, cyclic_pos, longest_match_length, num_pairs, num_avail, additional_offset;
  uint32_t reps[4], state, range, cache, cache_size;
  uint32_t _pad;
  uint64_t low, out_total;
} LzmaEncGpuSession;

/* Host only.  Bytes of a session's workspace slice: the probability cells, the
 * `matches` array, the hash (sized by dictSize, as in LzmaEncGpu_PlanBatch) and
 * the `son` ring sized by min(dictSize, src_cap) + 1; a multiple of 256.  0 for
 * props LzmaEncGpu_SessionInit refuses or src_cap >= 2^31. */
uint64_t LzmaEncGpu_SessionWorkspaceBytes(const CLzmaEncProps *props, uint64_t src_cap);
/* Host only.  LzmaEncGpu_DescFromProps' checks and results over *props
 * (SZ_ERROR_PARAM; SZ_ERROR_UNSUPPORTED for props that normalise to a normal
 * mode whatever LzmaEncGpu_SetModes says, with LzmaGpu_LastError() naming the
 * field, and for src_cap >= 2^31), then binds the caller's device buffers and
 * marks the slice as needing initialisation: the first round in which the
 * session has work clears its hash and sets its cells.  *s is written only on
 * SZ_OK, where props5 holds LzmaEnc_WriteProperties' 5 bytes. */
SRes LzmaEncGpu_SessionInit(LzmaEncGpuSession *s, const CLzmaEncProps *props, int writeEndMark,
                            const Byte *d_src, uint64_t src_cap, Byte *d_dst, uint64_t dst_cap,
                            void *d_workspace, Byte props5[5]);
/* Bytes of d_scratch for a round over n sessions: two counters and two index
 * lists (the sessions with work, and those of them whose slice needs
 * initialising). */
size_t LzmaEncGpu_SessionScratchBytes(size_t n);
/* One call per session, all in one round of launches on `stream`: a list pass
 * compacts the indices of the sessions with work (not finished, and finish set
 * or src_len - in_pos >= LZMA_ENC_GPU_SESSION_HOLD) into d_scratch, the whole
 * grid initialises the slices that need it, and one lane per listed session
 * encodes (lanes per 64-lane wave: 64, 32, 16 or LZMA_ENC_GPU_LANES_DEFAULT).
 * Waves past the list's end return at once, and a session without work is not
 * read beyond its record nor written at all.  d_scratch[0] (uint32_t) is the
 * number of sessions the round worked on.  No allocation, no synchronisation;
 * n == 0 is a no-op.  SZ_ERROR_FAIL without a device, SZ_ERROR_PARAM for n above
 * 2^31 - 1 or an unknown lanes value. */
SRes LzmaEncGpu_SessionEncodeBatch(LzmaEncGpuSession *d_sessions, size_t n, void *d_scratch,
                                   unsigned lanes, void *stream);
/* The round's first launch alone (what lzmaenc_session_bench.py times): clears
 * the two counters and compacts the lists into d_scratch. */
SRes LzmaEncGpu_SessionListPass(const LzmaEncGpuSession *d_sessions, size_t n, void *d_scratch,
                                void *stream);

/* LzmaEnc.h:38-59: the handle API the reference's `lzma e` is written
 * against, over one session.  LzmaEnc_Encode gathers inStream's reads into
 * pieces (a piece is complete at 4 KiB, at most 1 MiB, or at the stream's end),
 * appends each to a device buffer that starts at 1 MiB and doubles when full (a
 * new allocation and a device-to-device copy of the stream so far; dst and,
 * while the ring is sized by the source, the workspace slice grow with it),
 * advances the session once per piece and writes each round's new bytes to
 * outStream; a short write is SZ_ERROR_WRITE, a read error is returned as
 * it is.  progress is called once per round with (in_pos, out_pos), not every
 * 32 KiB; non-zero is SZ_ERROR_PROGRESS.  Props that select a normal mode: with
 * the modes mask admitting them the stream is read to its end and encoded by
 * LzmaEncode; otherwise SZ_ERROR_UNSUPPORTED, from SetProps already.
 * LzmaEnc_MemEncode is LzmaEncode with the handle's props.  alloc only holds
 * the handle. */
#ifndef __7Z_TYPES_H
typedef struct {   /* Types.h:137-160 */
  SRes (*Read)(void *p, void *buf, size_t *size);
  /* if (input(*size) != 0 && output(*size) == 0) means end_of_stream.
     (output(*size) < input(*size)) is allowed */
} ISeqInStream;
typedef struct {
  size_t (*Write)(void *p, const void *buf, size_t size);
  /* Returns: result - the number of actually written bytes.
     (result < size) means error */
} ISeqOutStream;
#endif
#ifndef __LZMA_ENC_H
typedef void *CLzmaEncHandle;
#endif
CLzmaEncHandle LzmaEnc_Create(ISzAlloc *alloc);
void LzmaEnc_Destroy(CLzmaEncHandle p, ISzAlloc *alloc, ISzAlloc *allocBig);
SRes LzmaEnc_SetProps(CLzmaEncHandle p, const CLzmaEncProps *props);
SRes LzmaEnc_WriteProperties(CLzmaEncHandle p, Byte *properties, SizeT *size);
SRes LzmaEnc_Encode(CLzmaEncHandle p, ISeqOutStream *outStream, ISeqInStream *inStream,
                    ICompressProgress *progress, ISzAlloc *alloc, ISzAlloc *allocBig);
SRes LzmaEnc_MemEncode(CLzmaEncHandle p, Byte *dest, SizeT *destLen, const Byte *src, SizeT srcLen,
                       int writeEndMark, ICompressProgress *progress, ISzAlloc *alloc,
                       ISzAlloc *allocBig);

/* ---------------------------------------------------------------- LZMA2 and xz writers */

/* LZMA2 in the reference's multi-threaded layout (Lzma2Enc.c:310-361): the
 * input is cut into blockSize pieces, every piece is an independent run of
 * chunks that starts with a dictionary reset, the runs are concatenated and one
 * 0x00 ends the stream.  A piece is one lane of an encode batch
 * (csrc/lzma2enc_device.h), on the fast path only (levels 0..4).  Per block the
 * outcome is MtCallbackImp_Code's over a buffer of dst_cap bytes, without the
 * final 0x00:
 *   SZ_OK                 dest_len bytes of chunks written; with dst_cap >=
 *                         Lzma2EncGpu_BlockBound(src_len) they are the bytes of
 *                         the reference's single-threaded Lzma2Enc_Encode of the
 *                         block alone, minus its last byte
 *   SZ_ERROR_OUTPUT_EOF   a chunk did not fit: dest_len = the bytes of the whole
 *                         chunks before it; bytes in [dest_len, dst_cap) are
 *                         unspecified
 *   SZ_ERROR_PARAM        what LzmaEncGpu_EncodeBatch refuses, and lc + lp > 4
 *   SZ_ERROR_UNSUPPORTED  src_len >= 2^31
 * Bytes of d_dst outside [dst_off, dst_off + dst_cap) are never written.  The
 * descriptors and results are the LZMA encoder's (write_end_mark is ignored). */

#ifndef __LZMA2_ENC_H
typedef struct {   /* 64 bytes, Lzma2Enc.h:13-19 */
  CLzmaEncProps lzmaProps;
  size_t blockSize;
  int numBlockThreads;
  int numTotalThreads;
} CLzma2EncProps;
typedef void *CLzma2EncHandle;
#endif

/* Lzma2Enc.c:168-234, of a build with threads (NUM_MT_CODER_THREADS_MAX 32) */
void Lzma2EncProps_Init(CLzma2EncProps *p);
void Lzma2EncProps_Normalize(CLzma2EncProps *p);

/* src_len + (src_len >> 10) + 16: the reference's destBlockSize (:471) */
size_t Lzma2EncGpu_BlockBound(size_t src_len);
/* Host only.  Lzma2Enc_SetProps' check (lc + lp > 4: SZ_ERROR_PARAM), then
 * LzmaEncGpu_DescFromProps' over the normalised lzmaProps.  On SZ_OK the props
 * fields of *desc are set and *prop is Lzma2Enc_WriteProperties' byte. */
SRes Lzma2EncGpu_DescFromProps(const CLzma2EncProps *props, LzmaEncGpuStreamDesc *desc, Byte *prop);
/* The same with the caller's mask of modes in place of LzmaEncGpu_GetModes()
 * (see LzmaEncGpu_DescFromPropsEx). */
SRes Lzma2EncGpu_DescFromPropsEx(const CLzma2EncProps *props, unsigned allowed,
                                 LzmaEncGpuStreamDesc *desc, Byte *prop);
/* LzmaEncGpu_PlanBatch over the LZMA2 slices (the LZMA slice plus the table
 * that holds the saved probability cells of the chunk in flight). */
SRes Lzma2EncGpu_PlanBatch(LzmaEncGpuStreamDesc *descs, size_t n, uint32_t *order,
                           uint64_t *workspace_bytes);
/* LzmaEncGpu_EncodeBatch's contract with blocks for streams. */
SRes Lzma2EncGpu_EncodeBatch(const LzmaEncGpuStreamDesc *d_descs, const uint32_t *d_order,
                             size_t n, const Byte *d_src, Byte *d_dst, void *d_workspace,
                             LzmaEncGpuResult *d_results, unsigned lanes, void *stream);
/* LzmaEncGpu_EncodeBatchHost's contract with blocks for streams. */
SRes Lzma2EncGpu_EncodeBatchHost(const LzmaEncGpuStreamDesc *descs, size_t n, const Byte *src,
                                 size_t src_size, Byte *dst, size_t dst_size,
                                 LzmaEncGpuResult *results, uint64_t workspace_limit);
/* One stream from the blocks of a finished batch, on the device: d_offsets[i]
 * (n + 1 entries of scratch) = the sum of d_results[0, i).dest_len, block i's
 * bytes go from d_slots + d_descs[i].dst_off to d_out + d_offsets[i], and 0x00
 * follows the last.  d_total: res = the first block's that is not SZ_OK (_pad =
 * its index), else SZ_ERROR_OUTPUT_EOF when the stream is longer than out_cap,
 * else SZ_OK; dest_len = the stream's length.  d_out is written only on SZ_OK.
 * All pointers device memory; asynchronous on `stream`; d_slots and d_out may
 * not overlap. */
SRes Lzma2EncGpu_Compact(const LzmaEncGpuStreamDesc *d_descs, const LzmaEncGpuResult *d_results,
                         size_t n, const Byte *d_slots, Byte *d_out, uint64_t out_cap,
                         uint64_t *d_offsets, LzmaEncGpuResult *d_total, void *stream);
/* One host buffer as one LZMA2 stream: cut by props->blockSize (after
 * Lzma2EncProps_Normalize), upload, one batch, compaction, download.  *destLen
 * in: capacity, out: the stream's length; *prop = the dictionary byte.  An empty
 * source gives the byte 00.  SZ_ERROR_PARAM / SZ_ERROR_UNSUPPORTED as
 * Lzma2EncGpu_DescFromProps (and a source of 2^31 blocks or more),
 * SZ_ERROR_OUTPUT_EOF when dest is short, SZ_ERROR_FAIL without a device. */
SRes LzmaGpu_Lzma2EncodeHost(Byte *dest, SizeT *destLen, const Byte *src, SizeT srcLen,
                             const CLzma2EncProps *props, Byte *prop);

/* Lzma2Enc.h:36-43.  Differences from the reference: Lzma2Enc_Encode reads the
 * input stream to its end before it encodes; numBlockThreads only selects the
 * layout (<= 1: the whole input is one block, the reference's
 * Lzma2Enc_EncodeMt1; > 1: blocks of blockSize); progress is called once per
 * finished block, after its bytes went through outStream; props off the fast
 * path give SZ_ERROR_UNSUPPORTED; alloc only holds the handle. */
CLzma2EncHandle Lzma2Enc_Create(ISzAlloc *alloc, ISzAlloc *allocBig);
void Lzma2Enc_Destroy(CLzma2EncHandle p);
SRes Lzma2Enc_SetProps(CLzma2EncHandle p, const CLzma2EncProps *props);
Byte Lzma2Enc_WriteProperties(CLzma2EncHandle p);
SRes Lzma2Enc_Encode(CLzma2EncHandle p, ISeqOutStream *outStream, ISeqInStream *inStream,
                     ICompressProgress *progress);

/* One xz stream from a host buffer: every piece of blockSize bytes is one xz
 * block with the filter chain LZMA2 only (a block header without size fields,
 * as Xz_Encode writes it, XzEnc.c:41-160), its data the piece's chunks and
 * 0x00.  The blocks are one encode batch; the block checks (LZMA_GPU_XZ_CHECK_*)
 * are computed on the device over the source pieces; headers, index and footer
 * are written on the host.  An empty source gives the 32-byte empty stream.
 * SZ_ERROR_UNSUPPORTED for another check id, SZ_ERROR_OUTPUT_EOF when dest is
 * short, else as LzmaGpu_Lzma2EncodeHost. */
SRes LzmaGpu_XzEncode(Byte *dest, SizeT *destLen, const Byte *src, SizeT srcLen,
                      const CLzma2EncProps *props, unsigned check_type);

/* One filter of an xz block's chain in front of LZMA2.  id: the ids of
 * LzmaGpuXzBlock.filter_id (3 delta, 4 x86, 5 PPC, 6 IA64, 7 ARM, 8 ARMT,
 * 9 SPARC); prop: the delta distance 1..256, or a branch converter's start
 * offset. */
typedef struct LzmaGpuXzFilter {   /* 8 bytes */
  uint32_t id;
  uint32_t prop;
} LzmaGpuXzFilter;
#define LZMA_GPU_XZ_ENC_FILTERS_MAX 3

/* LzmaGpu_XzEncode with a filter chain: every block lists `filters` in order,
 * then LZMA2.  Per block the chain runs first filter first in the encode
 * direction over a device copy of the piece, every filter restarting at the
 * block (x86 state 0, delta state 0, ip = the start offset), one batch per
 * filter of the chain; the LZMA2 batch encodes the filtered copy and the block
 * check is computed over the unfiltered source.  In the block header a delta
 * filter has one property byte (distance - 1), a branch converter none when
 * its start offset is 0 and four little-endian bytes otherwise.  Checked on
 * the host before any device work: SZ_ERROR_PARAM for more than
 * LZMA_GPU_XZ_ENC_FILTERS_MAX filters, a delta distance outside 1..256 or a
 * start offset that is no multiple of the converter's alignment (the reader's
 * rule: PPC, ARM and SPARC 4, IA64 16, ARMT 2, x86 1); SZ_ERROR_UNSUPPORTED
 * for another id.  num_filters == 0 is LzmaGpu_XzEncode, byte for byte. */
SRes LzmaGpu_XzEncodeEx(Byte *dest, SizeT *destLen, const Byte *src, SizeT srcLen,
                        const CLzma2EncProps *props, unsigned check_type,
                        const LzmaGpuXzFilter *filters, unsigned num_filters);

/* ---- Lzma86: LZMA with the x86 filter tried per stream (Lzma86.h) ----------
 * The header of an Lzma86 stream: byte 0 the filter flag (0 or 1), bytes 1..5
 * the LZMA props, bytes 6..13 the unpacked size, little-endian; the LZMA
 * stream follows without an end mark.  Lzma86_Encode with SZ_FILTER_AUTO
 * encodes the buffer with and without the filter and keeps the smaller result
 * (Lzma86Enc.c:59-101); in a batch every candidate is one more lane of the
 * same LzmaEncGpu_EncodeBatch launch, and the choice, the header and the move
 * of the chosen candidate into the caller's slot run on the device
 * (csrc/lzma86_device.h). */
#ifndef __LZMA86_H
#define LZMA86_SIZE_OFFSET (1 + 5)
#define LZMA86_HEADER_SIZE (LZMA86_SIZE_OFFSET + 8)
enum ESzFilterMode { SZ_FILTER_NO, SZ_FILTER_YES, SZ_FILTER_AUTO };
#endif

/* One stream of an Lzma86 batch (48 bytes): ranges of the caller's packed
 * buffers (any byte alignment) and Lzma86_Encode's level, dictSize and
 * filterMode.  Decoding reads the four ranges only. */
typedef struct Lzma86GpuStreamDesc {
  uint64_t src_off, src_len;
  uint64_t dst_off, dst_cap;
  int32_t level;
  uint32_t dictSize;
  int32_t filterMode;   /* SZ_FILTER_* */
  uint32_t reserved;    /* 0 */
} Lzma86GpuStreamDesc;

/* Per-stream outcome (24 bytes).  Encoding: Lzma86_Encode's return value and
 * *destLen, filter = the flag byte written, src_len = the stream's src_len.
 * Decoding: Lzma86_Decode's return value, *destLen and *srcLen (0 where the
 * reference leaves it untouched), filter = the flag byte read. */
typedef struct Lzma86GpuResult {
  int32_t res;
  uint32_t filter;
  uint64_t dest_len;
  uint64_t src_len;
} Lzma86GpuResult;

#define LZMA86_GPU_TIMINGS 1u      /* synchronise after every stage and fill stage_ns */
#define LZMA86_GPU_STAGE_FILTER 0  /* the copies of the sources and the x86 batch */
#define LZMA86_GPU_STAGE_ENCODE 1  /* the LzmaEncGpu_EncodeBatch launches */
#define LZMA86_GPU_STAGE_SELECT 2  /* choice, headers, gather */
#define LZMA86_GPU_STAGE_TOTAL 3   /* the call; set without TIMINGS too */
typedef struct Lzma86GpuStats {    /* 64 bytes */
  uint32_t flags;                  /* in: LZMA86_GPU_TIMINGS or 0 */
  uint32_t reserved;               /* 0 */
  uint64_t candidates;             /* lanes of the encode batch */
  uint64_t filtered;               /* streams that got a filtered candidate */
  uint64_t encode_launches;        /* 1 unless workspace_limit cuts the batch */
  uint64_t stage_ns[4];            /* LZMA86_GPU_STAGE_*: host clock, nanoseconds */
} Lzma86GpuStats;

/* Per stream the outcome is Lzma86_Encode's over a buffer of dst_cap bytes, bit
 * for bit: a dst_cap below 14 is SZ_ERROR_OUTPUT_EOF with dest_len 0 and nothing
 * written; each candidate is encoded into a capacity of dst_cap - 14; with AUTO
 * the filtered candidate wins only when it fits and is strictly smaller than
 * the unfiltered one (a tie goes to the unfiltered one, a lone fitting
 * candidate is taken); when no candidate fits: SZ_ERROR_OUTPUT_EOF, dest_len 14,
 * flag 0, the 14 header bytes written.  A filterMode other than NO and AUTO
 * acts as YES, as in the reference.  The filter is x86_Convert from ip 0 with a
 * fresh state over the whole source.  Differences: a level that normalises to a
 * normal mode is SZ_ERROR_UNSUPPORTED unless the modes mask admits it
 * (LzmaEncGpu_SetModes), a source of 2^31 bytes or more is SZ_ERROR_UNSUPPORTED,
 * a dictSize above 1 << 30 is SZ_ERROR_PARAM; these three leave dest_len 0 and
 * write nothing.  Bytes of dst outside [dst_off, dst_off + max(dest_len, 14))
 * are never written.
 *
 * Lzma86Gpu_EncodeScratch (host only): the bytes of d_scratch a batch needs --
 * the tables, the filtered copies of the sources, one slot of dst_cap - 14
 * bytes per candidate and the encoder's workspace; SZ_ERROR_PARAM for n above
 * 2^31 - 1.
 * Lzma86Gpu_EncodeBatch: `descs` is host memory (the plan is host work), every
 * other pointer device memory; d_scratch needs no initialisation.  One copy of
 * the tables, then on `stream`: the stage copies and one BcjGpu_X86Batch, one
 * LzmaEncGpu_EncodeBatch over all candidates (n lanes for NO and YES streams, 2
 * per AUTO stream, in the planner's order), select and gather.  SZ_OK if
 * everything was queued, SZ_ERROR_PARAM for a scratch_bytes below
 * Lzma86Gpu_EncodeScratch's, SZ_ERROR_FAIL without a device. */
SRes Lzma86Gpu_EncodeScratch(const Lzma86GpuStreamDesc *descs, size_t n, uint64_t *scratch_bytes);
SRes Lzma86Gpu_EncodeBatch(const Lzma86GpuStreamDesc *descs, size_t n, const Byte *d_src,
                           Byte *d_dst, void *d_scratch, uint64_t scratch_bytes,
                           Lzma86GpuResult *d_results, void *stream);
/* The same over host buffers: stages src and dst, plans as
 * LzmaEncGpu_EncodeBatchHost does (streams longest first; as many encode
 * launches as keep the encoder's workspace at or under workspace_limit, 0 = half
 * of the free device memory; a stream's two candidates share a launch).
 * SZ_ERROR_MEM if one stream's candidates alone exceed the limit or an
 * allocation fails, SZ_ERROR_PARAM for a range outside src / dst.  stats may
 * be NULL. */
SRes Lzma86Gpu_EncodeBatchHost(const Lzma86GpuStreamDesc *descs, size_t n, const Byte *src,
                               size_t src_size, Byte *dst, size_t dst_size,
                               Lzma86GpuResult *results, uint64_t workspace_limit,
                               Lzma86GpuStats *stats);

/* Per stream the outcome is Lzma86_Decode's: a src_len below 14 is
 * SZ_ERROR_INPUT_EOF, a flag byte above 1 SZ_ERROR_UNSUPPORTED (both with
 * dest_len and src_len 0); else LzmaDecode of the payload with LZMA_FINISH_ANY
 * into dst_cap bytes (src_len = 14 + the payload bytes read), and on SZ_OK with
 * flag 1 x86_Convert in the decode direction over the dest_len bytes decoded.
 * The host checks the headers: `headers` is host memory, 14 bytes per stream
 * (stream i's first min(14, src_len) bytes at headers + 14 * i).
 * Lzma86Gpu_DecodeScratch (host only): the bytes of d_scratch.
 * Lzma86Gpu_DecodeBatch: descs and headers host memory, every other pointer
 * device memory; on `stream`: one LzmaGpu_DecodeBatch over the payloads, the
 * finish kernel, one BcjGpu_X86Batch over the outputs of the streams flagged 1. */
SRes Lzma86Gpu_DecodeScratch(const Lzma86GpuStreamDesc *descs, size_t n, const Byte *headers,
                             uint64_t *scratch_bytes);
SRes Lzma86Gpu_DecodeBatch(const Lzma86GpuStreamDesc *descs, size_t n, const Byte *headers,
                           const Byte *d_src, Byte *d_dst, void *d_scratch,
                           uint64_t scratch_bytes, Lzma86GpuResult *d_results, void *stream);
/* The same over host buffers (the headers are read from src). */
SRes Lzma86Gpu_DecodeBatchHost(const Lzma86GpuStreamDesc *descs, size_t n, const Byte *src,
                               size_t src_size, Byte *dst, size_t dst_size,
                               Lzma86GpuResult *results);

/* Lzma86.h:71-107 as one-item calls of the host forms.  Differences from the
 * reference: those listed above; SZ_ERROR_FAIL without a device; on
 * SZ_ERROR_OUTPUT_EOF dest holds the 14 header bytes only. */
SRes Lzma86_Encode(Byte *dest, size_t *destLen, const Byte *src, size_t srcLen, int level,
                   UInt32 dictSize, int filterMode);
SRes Lzma86_GetUnpackSize(const Byte *src, SizeT srcLen, UInt64 *unpackSize);
SRes Lzma86_Decode(Byte *dest, SizeT *destLen, const Byte *src, SizeT *srcLen);

/* ---- 7z archives as folder batches ----------------
 * Replaces SzArEx_Open (7zIn.c:1314) + a SzArEx_Extract loop over every file
 * (7zIn.c:1322; ExtractAllFiles 7zIn.c:1405 in the fork): the header walk
 * runs on the host (an LZMA / LZMA2-packed header is decoded on the GPU),
 * every folder of the archive is one item of a single GPU batch, BCJ x86
 * and ARM folders go through the branch-converter kernels and every folder /
 * file CRC through one CRC-32 batch.  Folder shapes: Copy / LZMA / LZMA2,
 * optionally followed by BCJ x86 or ARM (CheckSupportedFolder, 7zDec.c:269;
 * ARM_Convert at ip 0, :449), and the reference's BCJ2 folder (four coders
 * in the one bind layout 7zDec.c:303-319 accepts): its three LZMA / LZMA2 /
 * Copy coders decode in the same batch and Bcj2Gpu_Batch merges them. */
typedef struct LzmaGpu7zFolder {   /* 80 bytes */
  uint64_t pack_off;     /* archive offset of the main coder's pack stream */
  uint64_t pack_size;
  uint64_t unpack_size;  /* SzFolder_GetUnpackSize */
  uint64_t dst_off;      /* offset of the folder's output in the extraction buffer */
  uint64_t method;       /* coder 0 method id (0 Copy, 0x030101 LZMA, 0x21 LZMA2) */
  uint32_t x86;          /* 1: a BCJ x86 coder follows */
  uint32_t supported;    /* SZ_OK, or the SRes the folder fails with before decoding */
  uint32_t crc_defined, crc;
  uint32_t first_file;   /* FolderStartFileIndex */
  uint32_t num_files;    /* NumUnpackStreams */
  uint32_t num_coders;
  uint32_t props_size;
  Byte props[8];
} LzmaGpu7zFolder;

typedef struct LzmaGpu7zFile {     /* 48 bytes */
  uint64_t size;
  uint64_t dst_off;      /* offset of the file's bytes in the extraction buffer */
  uint32_t folder;       /* FileIndexToFolderIndexMap: 0xFFFFFFFF = no data */
  uint32_t crc, crc_defined;
  uint32_t has_stream, is_dir;
  uint32_t name_off, name_len;  /* UTF-16 units into the names buffer (name_len counts the NUL) */
  uint32_t reserved;
} LzmaGpu7zFile;

/* SzArEx_Open: SZ_OK or its error (SZ_ERROR_NO_ARCHIVE, _UNSUPPORTED, _CRC,
 * _ARCHIVE, _INPUT_EOF, a packed header's decode error).  Fills up to
 * folder_cap / file_cap / names_cap entries (any pointer may be NULL); the
 * counts and *unpack_total (the extraction buffer size) are always set. */
SRes LzmaGpu_7zOpen(const Byte *archive, size_t size, LzmaGpu7zFolder *folders,
                    size_t folder_cap, size_t *n_folders, LzmaGpu7zFile *files, size_t file_cap,
                    size_t *n_files, UInt16 *names, size_t names_cap, size_t *names_len,
                    UInt64 *unpack_total);

/* Every folder decoded into dest (folders back to back, files at their
 * LzmaGpu7zFile.dst_off); *destLen in: capacity (SZ_ERROR_OUTPUT_EOF if
 * below unpack_total), out: unpack_total.  file_res[i] = what SzArEx_Extract
 * returns for file i with a fresh folder cache (SZ_OK, the folder's decode
 * error, SZ_ERROR_CRC, SZ_ERROR_FAIL).  Returns SzArEx_Open's error, else the
 * first file's non-OK result, else SZ_OK. */
SRes LzmaGpu_7zExtract(Byte *dest, SizeT *destLen, const Byte *archive, size_t size,
                       SRes *file_res, size_t file_cap);

/* The same with options.  flags = 0: exactly the two calls above.
 * LZMA_GPU_7Z_PPMD: method 0x030401 (PPMd7, the reference's compile-time
 * _7ZIP_PPMD_SUPPPORT, 7zDec.c:29-124, here a run-time choice) is a main
 * method wherever Copy / LZMA / LZMA2 are in the 1- and 2-coder shapes: alone
 * and under the x86 or ARM filter, in folders and in a packed header.  Its
 * checks before decoding are SzDecodePpmd's (props size != 5, order or memSize
 * out of range: SZ_ERROR_UNSUPPORTED); its streams decode in one
 * Ppmd7Gpu_DecodeBatch beside the LZMA batch.  Deviation from the reference's
 * switch: a PPMd coder inside a BCJ2 folder stays SZ_ERROR_UNSUPPORTED.  A flag
 * bit outside LZMA_GPU_7Z_KNOWN_FLAGS: SZ_ERROR_PARAM. */
#define LZMA_GPU_7Z_PPMD 1u
#define LZMA_GPU_7Z_KNOWN_FLAGS 1u
SRes LzmaGpu_7zOpenEx(const Byte *archive, size_t size, LzmaGpu7zFolder *folders,
                      size_t folder_cap, size_t *n_folders, LzmaGpu7zFile *files, size_t file_cap,
                      size_t *n_files, UInt16 *names, size_t names_cap, size_t *names_len,
                      UInt64 *unpack_total, unsigned flags);
SRes LzmaGpu_7zExtractEx(Byte *dest, SizeT *destLen, const Byte *archive, size_t size,
                         SRes *file_res, size_t file_cap, unsigned flags);

/* ---- 7z archive writer: every folder of an archive in one encode batch ----
 * The write side of the calls above.  The caller describes an archive as items
 * over one source buffer; every folder (one item, or a JOIN group) is one
 * stream of an LZMA, an LZMA2 (one stream per blockSize piece) or a PPMd7
 * encode batch, all folders of the archive at once; CRC-32 of every file and
 * the x86 / ARM filters run as batches over the uploaded source; the pack stage
 * (SzGpu_PackBatch) gathers the finished pieces into the pack area on the
 * device; the header is written on the host.  Format 7z 0.4 as the reference's
 * reader accepts it (7zIn.c, CheckSupportedFolder 7zDec.c:269-322): one coder,
 * or the main coder and a filter coder bound `in 1 <- out 0`, the filter at
 * ip 0 over the folder's whole data before the main coder.  Pack streams: LZMA
 * without end mark, LZMA2 in the multi-threaded layout with the final 0x00,
 * PPMd7 without end mark (props: order, memSize LE32), Copy the bytes.  Every
 * data file's CRC-32 is in SubStreamsInfo; no folder CRCs (except the packed
 * header's); no times, no attributes: the archive is a function of its inputs.
 * A BCJ2 folder (filter LZMA_GPU_7Z_FILTER_BCJ2 on an LZMA row) has the one
 * layout CheckSupportedFolder accepts (7zDec.c:303-319): coders 0, 1, 2 = the
 * JMP, CALL and main streams as LZMA, coder 3 = BCJ2 (0x0303011B, 4 in, 1 out),
 * bind pairs 5<-0, 4<-1, 3<-2, pack streams 2, 6, 1, 0 = the main LZMA stream,
 * the raw rc stream, the CALL and the JMP LZMA streams.  The main coder has the
 * row's props; the CALL and JMP coders the row's with lc 0, lp 2, pb 2 and the
 * dictionary min(the row's normalised dictSize, 1 MiB).  A branch is converted
 * when its target lies inside the folder's data (a JOIN group: the whole
 * group).  The split (Bcj2EncGpu_EncodeBatch's kernels) is out of place, so a
 * BCJ2 folder's source range may overlap another folder's.
 * Levels 5 and up need the modes switched on (LzmaEncGpu_SetModes).
 * Not written: BCJ2 over LZMA2, PPMd7 or Copy
 * rows, times and attributes, an archive that does not fit in device memory at
 * once. */

#define LZMA_GPU_7Z_ITEM_DIR 1u   /* a directory: size must be 0 */
#define LZMA_GPU_7Z_ITEM_JOIN 2u  /* continues the folder of the previous data item (solid) */

/* One archive entry.  size == 0 or DIR: no stream (kEmptyStream; kEmptyFile
 * when not a directory), in the caller's position.  JOIN: the bytes continue
 * the previous data item's folder: src_off must be where that item ended and
 * method the same index, else SZ_ERROR_PARAM (JOIN on an entry without data
 * means nothing). */
typedef struct LzmaGpu7zItem {     /* 32 bytes */
  uint64_t src_off, size;          /* range of the source buffer */
  uint32_t name_off, name_len;     /* UTF-16 units into names; name_len counts the NUL */
  uint32_t flags;                  /* LZMA_GPU_7Z_ITEM_* */
  uint32_t method;                 /* index into the method table */
} LzmaGpu7zItem;

/* One row of the method table.  method: 0 Copy, 0x030101 LZMA (props.lzmaProps),
 * 0x21 LZMA2 (props, blockSize after Lzma2EncProps_Normalize cuts the folder),
 * 0x030401 PPMd7 (ppmd_order 2..64, ppmd_mem_size 1<<11 .. 0xFFFFFFFF-36);
 * filter: 0 none, 4 x86, 7 ARM (the xz ids of BraGpu_Batch), 0x1B BCJ2 (LZMA
 * rows only: SZ_ERROR_UNSUPPORTED on another row; any other value
 * SZ_ERROR_PARAM).  The props go
 * through LzmaEncGpu_DescFromProps / Lzma2EncGpu_DescFromProps: their
 * SZ_ERROR_PARAM / SZ_ERROR_UNSUPPORTED (level 5 and up, unless
 * LzmaEncGpu_SetModes allows them) stand. */
#define LZMA_GPU_7Z_FILTER_BCJ2 0x1Bu
typedef struct LzmaGpu7zMethod {   /* 88 bytes */
  uint64_t method;
  uint32_t filter;
  uint32_t ppmd_order;
  uint32_t ppmd_mem_size;
  uint32_t reserved;               /* 0 */
  CLzma2EncProps props;
} LzmaGpu7zMethod;

#define LZMA_GPU_7Z_WRITE_ENCODE_HEADER 1u
#define LZMA_GPU_7Z_WRITE_TIMINGS 2u   /* synchronise after every stage and fill stats->stage_ns */
#define LZMA_GPU_7Z_WRITE_KNOWN_FLAGS 3u
typedef struct LzmaGpu7zWriteOptions {   /* 16 bytes */
  uint32_t flags;
  uint32_t reserved;               /* 0 */
  uint64_t workspace_limit;        /* as in the *BatchHost calls; 0 = half of the free memory */
} LzmaGpu7zWriteOptions;

#define LZMA_GPU_7Z_STAGE_UPLOAD 0
#define LZMA_GPU_7Z_STAGE_CRC 1
#define LZMA_GPU_7Z_STAGE_FILTER 2
#define LZMA_GPU_7Z_STAGE_ENCODE 3     /* the encode batches and the re-encode rounds */
#define LZMA_GPU_7Z_STAGE_PACK 4
#define LZMA_GPU_7Z_STAGE_DOWNLOAD 5   /* the pack area into dest */
#define LZMA_GPU_7Z_STAGE_HEADER 6     /* the header on the host; with ENCODE_HEADER its LZMA stream */
#define LZMA_GPU_7Z_STAGE_TOTAL 7      /* the call after the plan; set without TIMINGS too */
typedef struct LzmaGpu7zWriteStats {     /* 112 bytes */
  uint64_t folders;
  uint64_t pieces;                 /* encode pieces and Copy ranges: the pack stage's input */
  uint64_t reencoded;              /* streams encoded again with a larger slot */
  uint64_t pack_bytes;             /* the pack area (with the packed header's stream) */
  uint64_t header_bytes;           /* the header as it stands in the archive (the stub if packed) */
  uint64_t encode_launches;        /* encode batch launches for the folders (1 per kind unless
                                      workspace_limit cuts a batch or streams are re-encoded) */
  uint64_t stage_ns[8];            /* LZMA_GPU_7Z_STAGE_*: host clock, nanoseconds */
} LzmaGpu7zWriteStats;

/* Host only, no device.  Checks the method table (in order; the first error is
 * returned), then the items: SZ_ERROR_PARAM for an unknown method id or filter,
 * PPMd props out of range, a flag bit outside DIR | JOIN, a DIR with size != 0,
 * a method index, source range or name range out of bounds, a name_len of 0, a
 * bad JOIN, more than 2^32 - 2 items; SZ_ERROR_UNSUPPORTED for an LZMA or PPMd7
 * folder of 2^31 bytes or more.  Fills up to folder_cap folders (folders may be
 * NULL): unpack_size, dst_off (the folder's start in the source), method, x86,
 * num_coders (2 with a filter; x86 == 0 then means ARM; 4 for a BCJ2 folder,
 * which counts four pieces), props / props_size,
 * first_file (index of the folder's first item), num_files; pack_off, pack_size,
 * crc_defined, crc are 0.  *n_pieces: encode pieces + Copy ranges.
 * *dest_bound: a dest of that many bytes holds the archive whatever the data
 * (slots, not streams, counted; with or without ENCODE_HEADER). */
SRes LzmaGpu_7zWritePlan(const LzmaGpu7zItem *items, size_t n, size_t src_size, size_t names_len,
                         const LzmaGpu7zMethod *methods, size_t n_methods,
                         LzmaGpu7zFolder *folders, size_t folder_cap, size_t *n_folders,
                         size_t *n_pieces, uint64_t *dest_bound);

/* Host only.  flags 0: the header (kHeader, MainStreamsInfo, FilesInfo with
 * kEmptyStream / kEmptyFile / kName) for `folders` (as the plan gives them, with
 * pack_size set; pack streams back to back from pack_pos 0) and `items`;
 * file_crcs[i] = CRC-32 of item i's bytes (read for data items only).
 * LZMA_GPU_7Z_HEADER_STUB: the kEncodedHeader stub for folders[0] (n_folders 1:
 * the folder that packs the header, at pack_off, with pack_size, unpack_size,
 * props and its CRC when crc_defined); items are not read.
 * *header_len is always set; SZ_ERROR_OUTPUT_EOF when header_cap is below it
 * (header may be NULL).  sig32 (may be NULL): the 32-byte signature header for
 * this header after a pack area of pack_area_size bytes. */
#define LZMA_GPU_7Z_HEADER_STUB 1u
SRes LzmaGpu_7zWriteHeader(const LzmaGpu7zFolder *folders, size_t n_folders,
                           const LzmaGpu7zItem *items, size_t n, const uint32_t *file_crcs,
                           const UInt16 *names, size_t names_len, unsigned flags, Byte *header,
                           size_t header_cap, size_t *header_len, Byte *sig32,
                           uint64_t pack_area_size);

/* What the header needs beside LzmaGpu7zFolder for a four-coder (BCJ2) folder. */
typedef struct LzmaGpu7zBcj2Info {   /* 72 bytes */
  uint64_t pack_size[4];     /* main, rc, call, jump: the folder's pack streams in order */
  uint64_t unpack_size[3];   /* coders 0, 1, 2: the jump, call and main streams */
  Byte call_props[5], jump_props[5];
  Byte reserved[6];          /* 0 */
} LzmaGpu7zBcj2Info;
/* LzmaGpu_7zWriteHeader with bcj2[k] for the k-th folder of num_coders == 4, in
 * order (its pack_size is not read); fewer entries than such folders:
 * SZ_ERROR_PARAM.  LzmaGpu_7zWriteHeader is this call with no entries. */
SRes LzmaGpu_7zWriteHeaderEx(const LzmaGpu7zFolder *folders, size_t n_folders,
                             const LzmaGpu7zItem *items, size_t n, const uint32_t *file_crcs,
                             const UInt16 *names, size_t names_len, unsigned flags,
                             const LzmaGpu7zBcj2Info *bcj2, size_t n_bcj2, Byte *header,
                             size_t header_cap, size_t *header_len, Byte *sig32,
                             uint64_t pack_area_size);

/* The whole archive from host memory: upload, CRC batch, filter batches (in
 * place, after the CRCs; a filtered folder's source range may not overlap
 * another folder's: SZ_ERROR_PARAM; the BCJ2 split writes its four streams behind
 * the uploaded source and its lengths come back in one small copy; its three
 * LZMA streams per folder join the LZMA batch and rc is a Copy piece), the LZMA,
 * LZMA2 and PPMd7 batches (each cut
 * by workspace_limit as the *BatchHost calls are), pack, one download of the
 * pack area and one of the pack sizes, header.  LZMA and PPMd7 have no tight
 * bound: a stream gets a slot of len + len / 128 + 64 bytes first (incompressible
 * streams above about 9 KiB outgrow it: LZMA's fast mode adds 1.45 %); the streams
 * that report SZ_ERROR_OUTPUT_EOF are encoded again in one more batch per kind,
 * at most twice (PPMd7 with its packed_len, LZMA with len + len / 3 + 128, then
 * 2 * len + 1024), after which the call fails with SZ_ERROR_FAIL.
 * ENCODE_HEADER: the header is one more LZMA folder (level 4, lc3 lp0 pb2, with
 * a folder CRC) after the pack area, encoded by the same batch path in a
 * second launch of one stream -- one lane, about 0.5 MB/s -- and the archive
 * ends in the kEncodedHeader stub.
 * *destLen in: capacity, out: the archive's size.  SZ_ERROR_OUTPUT_EOF when dest
 * is short: *destLen = the needed size and dest is not written.  The plan's
 * errors come before anything touches the device; SZ_ERROR_FAIL without a
 * device (there is no CPU fallback).  options and stats may be NULL. */
SRes LzmaGpu_7zWrite(Byte *dest, SizeT *destLen, const Byte *src, size_t src_size,
                     const LzmaGpu7zItem *items, size_t n, const UInt16 *names, size_t names_len,
                     const LzmaGpu7zMethod *methods, size_t n_methods,
                     const LzmaGpu7zWriteOptions *options, LzmaGpu7zWriteStats *stats);

/* The pack stage on the device (csrc/sevenz_pack_device.h).  Piece i's bytes
 * start at bases[base] + off; its length is `len` for a Copy range, else the
 * dest_len of result `slot` of its kind's result array.  Pieces of a folder are
 * consecutive.  LAST: a 0x00 follows the piece (the last of an LZMA2 folder). */
#define LZMA_GPU_7Z_PACK_COPY 0u
#define LZMA_GPU_7Z_PACK_LZMA 1u
#define LZMA_GPU_7Z_PACK_LZMA2 2u
#define LZMA_GPU_7Z_PACK_PPMD 3u
#define LZMA_GPU_7Z_PACK_LAST 1u
#define LZMA_GPU_7Z_PACK_BASES 4
typedef struct SzGpuPackPiece {   /* 32 bytes */
  uint64_t off;
  uint64_t len;      /* Copy only */
  uint32_t slot;
  uint32_t folder;
  uint16_t kind;     /* LZMA_GPU_7Z_PACK_COPY .. PPMD */
  uint16_t base;     /* index into bases */
  uint32_t flags;    /* LZMA_GPU_7Z_PACK_LAST */
} SzGpuPackPiece;

/* All pointers device memory, bases 16-byte aligned (unused ones NULL); d_out
 * may not overlap a base.  d_scratch: SzGpu_PackScratch(n) uint64.  Outputs:
 * d_piece_off[i] = piece i's place in d_out (an exclusive scan of the lengths,
 * LAST pieces counting one more), d_folder_size[f] = folder f's pack size (only
 * on SZ_OK; a folder without pieces is not written), d_total: res = the first
 * piece's that is not SZ_OK (_pad = its index; SZ_ERROR_PARAM for a kind, base,
 * slot or folder out of range), else SZ_ERROR_OUTPUT_EOF when the total exceeds
 * out_cap, else SZ_OK; dest_len = the total.  d_out is written only on SZ_OK,
 * and then only in [0, total). */
typedef struct SzGpuPackArgs {    /* 152 bytes */
  const SzGpuPackPiece *d_pieces;
  uint64_t n, n_folders;
  const Byte *bases[LZMA_GPU_7Z_PACK_BASES];
  const LzmaEncGpuResult *d_lzma;
  uint64_t n_lzma;
  const LzmaEncGpuResult *d_lzma2;
  uint64_t n_lzma2;
  const Ppmd7GpuEncResult *d_ppmd;
  uint64_t n_ppmd;
  Byte *d_out;
  uint64_t out_cap;
  uint64_t *d_scratch, *d_piece_off, *d_folder_size;
  LzmaEncGpuResult *d_total;
} SzGpuPackArgs;
size_t SzGpu_PackScratch(size_t n);
/* Four launches on `stream`, asynchronous.  SZ_OK if they were queued,
 * SZ_ERROR_PARAM for n above 2^31 - 1, SZ_ERROR_FAIL without a device. */
SRes SzGpu_PackBatch(const SzGpuPackArgs *args, void *stream);

/* Device / diagnostics. */
int LzmaGpu_DeviceCount(void);
const char *LzmaGpu_LastError(void);
const char *LzmaGpu_Version(void);

#ifdef __cplusplus
}
#endif

#endif /* LZMA_GPU_H */
