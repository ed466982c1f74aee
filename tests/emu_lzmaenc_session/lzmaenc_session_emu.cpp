// Host build of the encoder sessions: LzmaEnc::session_call of
// csrc/lzmaenc_device.h on the public LzmaEncGpuSession record, one round as
// lzmaenc_session_kernels.hip runs it (the list pass's test, the slice's
// initialisation when the record asks for it, the call).
//   shared library: for tests/test_lzmaenc_session_emu.py (ctypes)
//   -DLZMAENC_SESSION_EMU_MAIN: a stand-alone program over a schedule file, for
//     the sanitizer run (tests/lzmaenc_session_cases.py write_schedule_file)
//
// A session lives in exact-size heap blocks: the slice (poisoned before it is
// initialised), dst (dst_cap bytes) and, with `fresh` set, a new copy of exactly
// the supplied prefix of the source for every call, so that a sanitizer sees any
// access outside them.  The record itself is poisoned before it is bound.
#define LZGPU_HOST_EMU 1
#include "lzmaenc_device.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/lzma_gpu.h"

static_assert(LZMA_ENC_GPU_SESSION_HOLD == lzenc::kSessionHold, "the published hold");

namespace {

struct Session {
  LzmaEncGpuSession s;
  uint8_t* slice;
  uint8_t* dst;
  uint64_t slice_bytes, rounds_worked;
  uint32_t crc[256];
};

uint64_t fnv(const uint8_t* p, uint64_t n) {
  uint64_t h = 1469598103934665603ull;
  for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

}  // namespace

// Props as lzmaenc_emu_encode builds them.  NULL with *res set when the props or
// the source's room are refused (LzmaEncGpu_SessionInit's results).
extern "C" void* lzs_new(int level, uint32_t dict_size, int lc, int lp, int pb, int fb, uint32_t mc,
                         int algo, int bt_mode, int end_mark, uint64_t src_cap, uint64_t dst_cap,
                         int poison, uint8_t* props5, int* res) {
  lzenc::EncProps props;
  lzenc::props_init(&props);
  props.level = level;
  props.dictSize = dict_size;
  props.lc = lc;
  props.lp = lp;
  props.pb = pb;
  props.fb = fb;
  props.mc = mc;
  props.algo = algo;
  props.btMode = bt_mode;
  props.numThreads = 1;
  lzenc::Params q;
  *res = lzenc::params_from_props(&props, end_mark, &q);
  if (*res != lzenc::kOk) return nullptr;
  *res = lzenc::check_params(q, src_cap);
  if (*res != lzenc::kOk) return nullptr;
  lzenc::write_props5(q, props5);
  Session* h = (Session*)malloc(sizeof(Session));
  memset(h, poison, sizeof(Session));
  h->slice_bytes = lzenc::lzmaenc_layout(q, src_cap).bytes;
  h->slice = (uint8_t*)aligned_alloc(256, h->slice_bytes);
  memset(h->slice, poison, h->slice_bytes);
  h->dst = (uint8_t*)malloc(dst_cap ? dst_cap : 1);
  memset(h->dst, 0xEE, dst_cap ? dst_cap : 1);
  h->rounds_worked = 0;
  for (uint32_t v = 0; v < 256; ++v) h->crc[v] = lzenc::crc_entry(v);
  lzenc::session_bind(&h->s, q, (const uint8_t*)nullptr, src_cap, h->dst, dst_cap, h->slice);
  return h;
}

extern "C" void lzs_free(void* hp) {
  Session* h = (Session*)hp;
  free(h->slice);
  free(h->dst);
  free(h);
}

extern "C" LzmaEncGpuSession* lzs_record(void* hp) { return &((Session*)hp)->s; }
extern "C" const uint8_t* lzs_dst(void* hp) { return ((Session*)hp)->dst; }
extern "C" uint64_t lzs_slice_bytes(void* hp) { return ((Session*)hp)->slice_bytes; }
extern "C" uint64_t lzs_slice_sum(void* hp) {
  Session* h = (Session*)hp;
  return fnv(h->slice, h->slice_bytes);
}
extern "C" uint64_t lzs_rounds_worked(void* hp) { return ((Session*)hp)->rounds_worked; }

// One round for one session: src[0, src_len) is the stream so far.  Returns 1
// when the session had work (the list pass would have listed it), else 0, in
// which case nothing but the per-call fields of the record was touched.
extern "C" int lzs_call(void* hp, const uint8_t* src, uint64_t src_len, int finish,
                        uint64_t in_budget, uint32_t hold, int fresh) {
  Session* h = (Session*)hp;
  uint8_t* copy = nullptr;
  if (fresh) {
    copy = (uint8_t*)malloc(src_len ? src_len : 1);
    memcpy(copy, src, src_len);
    src = copy;
  }
  h->s.src = src;
  h->s.src_len = src_len;
  h->s.finish = finish ? 1u : 0u;
  h->s.in_budget = in_budget;
  const bool work = lzenc::session_has_work(h->s, hold);
  if (work) {
    if (lzenc::session_wants_init(h->s, hold))
      lzenc::lzmaenc_init_slice(h->slice, lzenc::lzmaenc_layout(lzenc::session_params(h->s),
                                                                 h->s.src_cap), 0, 1);
    lzenc::LzmaEnc e;
    e.session_call(h->s, h->crc, hold);
    h->rounds_worked++;
  }
  h->s.src = nullptr;
  free(copy);
  return work ? 1 : 0;
}

// A whole stream through one session by a piece schedule: after piece i the
// call sees the first pieces[0] + .. + pieces[i] bytes (not final); then the
// final call over all n bytes.  A call that ends with BUDGET is repeated with
// the same arguments.  The published guarantees are checked after every call;
// the first that fails is the (negative) return value:
//   -1  a non-final call ended with neither BUDGET nor src_len - in_pos < HOLD
//   -2  output or input consumed before HOLD bytes were supplied
//   -3  in_pos / out_pos went backwards, or past src_len / dst_cap
//   -4  bytes below an earlier out_pos changed
//   -5  a call with a budget advanced in_pos by less than the budget or by
//       budget + 32 KiB + 273 or more, or ended BUDGET with finish set wrongly
//   -6  a call after the end changed the record or dst
//   -7  a session without work was touched
//   -8  the final call did not finish
// 0 on success: *res, *out_len = the session's, out[0, min(out_len, dst_cap))
// from the caller's own view of dst (lzs_dst).  calls / budget_calls count.
extern "C" int lzs_run(void* hp, const uint8_t* data, uint64_t n, const uint32_t* pieces,
                       uint32_t n_pieces, uint64_t in_budget, uint32_t hold, int fresh, int* res,
                       uint64_t* out_len, uint64_t* calls, uint64_t* budget_calls) {
  Session* h = (Session*)hp;
  const bool published = hold == LZMA_ENC_GPU_SESSION_HOLD;
  uint8_t* shadow = (uint8_t*)malloc(h->s.dst_cap ? h->s.dst_cap : 1);
  uint64_t supplied = 0, prev_in = 0, prev_out = 0;
  int bad = 0;
  *calls = *budget_calls = 0;
  for (uint32_t i = 0; i <= n_pieces && !bad; ++i) {
    const bool last = i == n_pieces;
    supplied = last ? n : supplied + pieces[i];
    if (supplied > n) supplied = n;
    for (;;) {
      const LzmaEncGpuSession before = h->s;
      const uint64_t sum_before = h->s.needs_init ? 0 : fnv(h->slice, 64);
      const int worked = lzs_call(h, data, supplied, last, in_budget, hold, fresh);
      ++*calls;
      const LzmaEncGpuSession& s = h->s;
      if (!worked) {
        if (s.in_pos != before.in_pos || s.out_pos != before.out_pos ||
            s.needs_init != before.needs_init || s.low != before.low ||
            (!s.needs_init && fnv(h->slice, 64) != sum_before))
          bad = -7;
      }
      if (s.in_pos < prev_in || s.out_pos < prev_out || s.in_pos > supplied ||
          s.out_pos > s.dst_cap)
        bad = -3;
      else if (memcmp(shadow, h->dst, prev_out) != 0)
        bad = -4;
      if (bad) break;
      memcpy(shadow + prev_out, h->dst + prev_out, s.out_pos - prev_out);
      const uint64_t advance = s.in_pos - prev_in;
      prev_in = s.in_pos;
      prev_out = s.out_pos;
      if (s.finished) break;
      if (s.status == LZMA_ENC_GPU_SESSION_BUDGET) {
        ++*budget_calls;
        if (in_budget == 0 || advance < in_budget || advance >= in_budget + (1u << 15) + 273)
          bad = -5;
        if (bad) break;
        continue;
      }
      if (last) bad = -8;
      else if (published && supplied - s.in_pos >= LZMA_ENC_GPU_SESSION_HOLD) bad = -1;
      else if (published && supplied < LZMA_ENC_GPU_SESSION_HOLD && (s.in_pos || s.out_pos))
        bad = -2;
      break;
    }
    if (h->s.finished) break;
  }
  if (!bad && !h->s.finished) bad = -8;
  if (!bad) {
    // done or dead: one more call, final or not, changes nothing
    for (int fin = 0; fin < 2 && !bad; ++fin) {
      const LzmaEncGpuSession before = h->s;
      lzs_call(h, data, n, fin, 0, hold, fresh);
      LzmaEncGpuSession after = h->s;
      after.src_len = before.src_len;  // the caller's own per-call fields
      after.finish = before.finish;
      after.in_budget = before.in_budget;
      if (memcmp(&after, &before, sizeof(after)) != 0 ||
          memcmp(shadow, h->dst, prev_out) != 0)
        bad = -6;
    }
  }
  free(shadow);
  *res = h->s.res;
  *out_len = h->s.out_pos;
  return bad;
}

// Every split of data[0, n) into two calls -- k bytes not final, then all n
// final -- for k = 0 .. n, against the one-shot stream `want`.  Returns the
// number of k whose bytes, length or res differ (or a negative lzs_run code).
extern "C" int64_t lzs_every_split(const uint8_t* data, uint64_t n, int level, uint32_t dict_size,
                                   int fb, uint32_t hold, const uint8_t* want, uint64_t want_len) {
  int64_t differ = 0;
  for (uint64_t k = 0; k <= n; ++k) {
    uint8_t props5[5];
    int res = 0;
    void* h = lzs_new(level, dict_size, -1, -1, -1, fb, 0, -1, -1, 0, n, want_len + 64,
                      int(0x3C + (k & 1) * 0x69), props5, &res);
    if (!h) return -100;
    const uint32_t piece = uint32_t(k);
    uint64_t out_len = 0, calls = 0, budget_calls = 0;
    const int bad = lzs_run(h, data, n, &piece, 1, 0, hold, 0, &res, &out_len, &calls,
                            &budget_calls);
    if (bad) {
      lzs_free(h);
      return bad;
    }
    if (res != 0 || out_len != want_len || memcmp(lzs_dst(h), want, want_len) != 0) ++differ;
    lzs_free(h);
  }
  return differ;
}

#ifdef LZMAENC_SESSION_EMU_MAIN
// Records of  i32 level, u32 dict, i32 lc, lp, pb, fb, u32 mc, i32 end_mark,
// u64 n, u64 dst_cap, u64 in_budget, u32 n_pieces, i32 res, u64 out_len, then
// n_pieces u32 piece sizes, n source bytes and min(out_len, dst_cap) expected
// bytes.  Every record runs twice, with two poison bytes and fresh exact-size
// copies of the supplied prefix for every call.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned count = 0, wrong = 0;
  for (;;) {
    int32_t a[8];
    uint64_t n, dst_cap, in_budget, exp_len;
    uint32_t n_pieces;
    int32_t exp_res;
    if (fread(a, 4, 8, f) != 8) break;
    if (fread(&n, 8, 1, f) != 1 || fread(&dst_cap, 8, 1, f) != 1 ||
        fread(&in_budget, 8, 1, f) != 1 || fread(&n_pieces, 4, 1, f) != 1 ||
        fread(&exp_res, 4, 1, f) != 1 || fread(&exp_len, 8, 1, f) != 1)
      return 2;
    uint32_t* pieces = (uint32_t*)malloc(n_pieces ? n_pieces * 4 : 4);
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    uint8_t* want = (uint8_t*)malloc(exp_len ? exp_len : 1);
    if (fread(pieces, 4, n_pieces, f) != n_pieces || fread(data, 1, n, f) != n ||
        fread(want, 1, exp_len, f) != exp_len)
      return 2;
    for (int pass = 0; pass < 2; ++pass) {
      uint8_t props5[5];
      int res = 0;
      void* h = lzs_new(a[0], uint32_t(a[1]), a[2], a[3], a[4], a[5], uint32_t(a[6]), -1, -1, a[7],
                        n, dst_cap, pass ? 0xA5 : 0x3C, props5, &res);
      if (!h) return 2;
      uint64_t out_len = 0, calls = 0, budget_calls = 0;
      const int bad = lzs_run(h, data, n, pieces, n_pieces, in_budget, LZMA_ENC_GPU_SESSION_HOLD, 1,
                              &res, &out_len, &calls, &budget_calls);
      if (bad || res != exp_res || out_len != exp_len || memcmp(lzs_dst(h), want, exp_len) != 0) {
        printf("record %u pass %d: check %d, got (%d, %llu) want (%d, %llu)\n", count, pass, bad,
               res, (unsigned long long)out_len, exp_res, (unsigned long long)exp_len);
        ++wrong;
      }
      lzs_free(h);
    }
    free(pieces);
    free(data);
    free(want);
    ++count;
  }
  fclose(f);
  printf("%u records, %u mismatches\n", count, wrong);
  return wrong ? 1 : 0;
}
#endif
