// sliced_device.h -- the per-stream code of the time-sliced batch kernels
// (sliced.hip): the decoder reset and one round's call on a spilled session.
// Plain device code with no HIP runtime, shared with the test-only host
// emulation build (tests/emu) like lzma_lane.h.
#pragma once

#include "lzma_lane.h"

namespace lzgpu {

// LzmaDec_Init on a bound session (LzmaDec.c:685-705 via LzmaDec_InitDicAndState)
__device__ __forceinline__ void sliced_reset(LzgpuSession& q) {
  q.dic_pos = 0;
  q.in_used = 0;  // consumed so far (cumulative over rounds)
  q.range = q.code = 0;
  q.processed_pos = q.check_dic_size = 0;
  q.state = 0;
  q.reps[0] = q.reps[1] = q.reps[2] = q.reps[3] = 1;
  q.remain_len = 0;
  q.need_flush = 1;       // range coder init pending
  q.need_init_state = 1;  // probabilities initialised by the first call
  q.temp_buf_size = 0;
}

// One round's call on one stream; true when the stream is finished (its
// LzmaGpuResult in r).  The call is LzmaDec_DecodeToDic(dicLimit = dicPos +
// slice, LZMA_FINISH_ANY), or with the stream's finish mode once the limit is
// dst_cap.
template <uint32_t M, class Lo>
__device__ __forceinline__ bool sliced_step(LzgpuSession& q, uint64_t slice, Lo lo,
                                            LzmaGpuResult& r) {
  const uint64_t cap = q.dic_buf_size;
  uint64_t lim = (cap - q.dic_pos > slice) ? q.dic_pos + slice : cap;
  int res, st;
  for (int pass = 0;; ++pass) {
    const int fin = lim == cap ? q.finish_mode : int(kFinAny);
    uint64_t used = q.in_len - q.in_used;
    st = kStNone;
    res = session_to_dic<M>(q, lim, (const gbyte*)(q.in + q.in_used), used, fin, st, lo);
    q.in_used += used;
    if (res != kErrData || pass != 0) break;
    // The reference reports a data error with the state of the DecodeReal /
    // DecodeReal2 call it happened in rolled back (LzmaDec.c:797, 826: locals
    // not written back), so destLen / srcLen name that call's start, and a
    // round's call boundaries are starts a one-call LzmaDecode does not have.
    // A corrupt stream is decoded again from its start as that one call, whose
    // result is LzmaDecode's (once per corrupt stream; other streams' rounds
    // stay bounded).
    sliced_reset(q);
    lim = cap;
  }
  const bool done = res != kOk || st == kStDoneMark || st == kStMoreInput || lim == cap;
  if (done) {
    r.res = (res == kOk && st == kStMoreInput) ? int(kErrInputEof) : res;
    r.status = st;
    r.dest_len = q.dic_pos;
    r.src_len = q.in_used;
  }
  return done;
}

}  // namespace lzgpu
