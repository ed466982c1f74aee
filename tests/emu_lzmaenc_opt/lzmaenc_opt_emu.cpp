// Host build of csrc/lzmaenc_device.h's normal-mode encoder (LzmaEncNormal:
// the optimal parser and / or the Bt4 finder), one stream.
//   shared library: lzmaenc_opt_emu_encode() for tests/test_lzmaenc_opt_emu.py
//   -DLZMAENC_OPT_EMU_MAIN: a stand-alone program over a case file, for the
//     sanitizer run (tests/lzmaenc_opt_cases.py write_case_file): records of
//     i32 level, u32 dict, i32 lc, lp, pb, fb, u32 mc, i32 algo, i32 bt_mode,
//     i32 num_hash_bytes, i32 end_mark, u32 allowed, u64 src_len, u64 dst_cap,
//     i32 res, u64 dest_len, 5 props bytes, then src_len source bytes and
//     dest_len expected bytes.  Every record runs twice, with two workspace
//     poison bytes, and both runs must give the expected bytes.
#define LZGPU_HOST_EMU 1
#include "lzmaenc_device.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// As lzmaenc_emu_encode, with the props' numHashBytes and the mask of modes
// the caller allows (lzenc::kModeOptimal | lzenc::kModeBt4).  Mode 0 runs the
// fast-path struct, every other mode the normal one, as the kernels do.  The
// workspace is a heap block of exactly the slice size filled with `poison`.
extern "C" int lzmaenc_opt_emu_encode(const uint8_t* src, uint64_t src_len, uint8_t* dst,
                                      uint64_t dst_cap, int level, uint32_t dict_size, int lc,
                                      int lp, int pb, int fb, uint32_t mc, int algo, int bt_mode,
                                      int num_hash_bytes, int end_mark, uint32_t allowed, int poison,
                                      uint8_t* props5, uint64_t* dest_len) {
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
  props.numHashBytes = num_hash_bytes;
  props.numThreads = 1;
  lzenc::Params q;
  *dest_len = 0;
  int32_t res = lzenc::params_from_props_ex(&props, end_mark, allowed, &q);
  if (res != lzenc::kOk) return res;
  lzenc::write_props5(q, props5);
  res = lzenc::check_params(q, src_len);
  if (res != lzenc::kOk) return res;
  const lzenc::Layout l = lzenc::lzmaenc_layout(q, src_len);
  uint8_t* slice = (uint8_t*)malloc(l.bytes);
  if (!slice) return 2;
  memset(slice, poison, l.bytes);
  lzenc::lzmaenc_init_slice(slice, l, 0, 1);
  uint32_t crc[256], prob_prices[lzenc::kProbPricesWords];
  for (uint32_t v = 0; v < 256; ++v) crc[v] = lzenc::crc_entry(v);
  for (uint32_t v = 0; v < lzenc::kProbPricesWords; ++v) prob_prices[v] = lzenc::prob_price_entry(v);
  lzenc::Out o;
  if (lzenc::mode_of(q) == 0) {
    lzenc::LzmaEnc e;
    o = e.encode(src, uint32_t(src_len), dst, dst_cap, q, slice, l, crc);
  } else {
    lzenc::LzmaEncNormal e;
    o = e.encode(src, uint32_t(src_len), dst, dst_cap, q, slice, l, crc, prob_prices);
  }
  free(slice);
  *dest_len = o.dest_len;
  return o.res;
}

extern "C" uint64_t lzmaenc_opt_emu_slice_bytes(uint32_t dict_size, uint32_t lc, uint32_t lp,
                                                uint32_t pb, uint32_t algo, uint32_t bt,
                                                uint64_t src_len) {
  lzenc::Params q{dict_size, lc, lp, pb, 5, 0, 0};
  q.algo = algo;
  q.bt = bt;
  return lzenc::lzmaenc_layout(q, src_len).bytes;
}

// ProbPrices[i] (LzmaEnc_InitPriceTables), for a check against the table's known values
extern "C" uint32_t lzmaenc_opt_emu_prob_price(uint32_t i) { return lzenc::prob_price_entry(i); }

#ifdef LZMAENC_OPT_EMU_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned n = 0, bad = 0;
  for (;;) {
    int32_t h[12];
    uint64_t src_len, dst_cap, exp_dest;
    int32_t exp_res;
    uint8_t exp_props[5];
    if (fread(h, 4, 12, f) != 12) break;
    if (fread(&src_len, 8, 1, f) != 1 || fread(&dst_cap, 8, 1, f) != 1 ||
        fread(&exp_res, 4, 1, f) != 1 || fread(&exp_dest, 8, 1, f) != 1 ||
        fread(exp_props, 1, 5, f) != 5)
      return 2;
    // exact-size blocks: an over-read of the source or an over-write of the
    // destination is the sanitizer's to report
    uint8_t* src = (uint8_t*)malloc(src_len ? src_len : 1);
    uint8_t* want = (uint8_t*)malloc(exp_dest ? exp_dest : 1);
    if (fread(src, 1, src_len, f) != src_len || fread(want, 1, exp_dest, f) != exp_dest) return 2;
    for (int pass = 0; pass < 2; ++pass) {
      uint8_t* dst = (uint8_t*)malloc(dst_cap ? dst_cap : 1);
      uint8_t props5[5] = {0, 0, 0, 0, 0};
      uint64_t dl = 0;
      const int res = lzmaenc_opt_emu_encode(src, src_len, dst, dst_cap, h[0], uint32_t(h[1]), h[2],
                                             h[3], h[4], h[5], uint32_t(h[6]), h[7], h[8], h[9],
                                             h[10], uint32_t(h[11]), pass ? 0xA5 : 0x3C, props5, &dl);
      const bool props_ok = (res == 4 || res == 5) || memcmp(props5, exp_props, 5) == 0;
      if (res != exp_res || dl != exp_dest || !props_ok || memcmp(dst, want, exp_dest) != 0) {
        printf("case %u pass %d: got (%d, %llu) want (%d, %llu)\n", n, pass, res,
               (unsigned long long)dl, exp_res, (unsigned long long)exp_dest);
        ++bad;
      }
      free(dst);
    }
    free(src);
    free(want);
    ++n;
  }
  fclose(f);
  printf("%u cases, %u mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
