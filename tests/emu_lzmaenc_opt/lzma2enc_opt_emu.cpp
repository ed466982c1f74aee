// Host build of csrc/lzma2enc_device.h's normal-mode block encoder
// (Lzma2EncNormal), one block.
//   shared library: lzma2enc_opt_emu_encode() for tests/test_lzmaenc_opt_emu.py
//   -DLZMA2ENC_OPT_EMU_MAIN: a stand-alone program over a case file, for the
//     sanitizer run (tests/lzma2enc_opt_cases.py write_case_file): records of
//     i32 level, u32 dict, i32 lc, lp, pb, u32 allowed, u64 src_len, u64 dst_cap,
//     i32 res, u64 dest_len, then src_len source bytes and dest_len expected
//     bytes.  Every record runs twice, with two workspace poison bytes.
#define LZGPU_HOST_EMU 1
#include "lzma2enc_device.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

// As lzma2enc_emu_encode, with the mask of modes the caller allows.  Mode 0
// runs the fast-path struct, every other mode the normal one, as the kernels do.
extern "C" int lzma2enc_opt_emu_encode(const uint8_t* src, uint64_t src_len, uint8_t* dst,
                                       uint64_t dst_cap, int level, uint32_t dict_size, int lc,
                                       int lp, int pb, uint32_t allowed, int poison, uint8_t* prop,
                                       uint64_t* dest_len) {
  lzenc::Enc2Props props;
  lzenc::props2_init(&props);
  props.lzmaProps.level = level;
  props.lzmaProps.dictSize = dict_size;
  props.lzmaProps.lc = lc;
  props.lzmaProps.lp = lp;
  props.lzmaProps.pb = pb;
  props.lzmaProps.numThreads = 1;
  props.numBlockThreads = 1;
  props.numTotalThreads = 1;
  lzenc::Params q;
  *dest_len = 0;
  int32_t res = lzenc::lzma2_params_from_props_ex(&props, allowed, &q, prop);
  if (res != lzenc::kOk) return res;
  res = lzenc::lzma2_check_params(q, src_len);
  if (res != lzenc::kOk) return res;
  const lzenc::Layout2 m = lzenc::lzma2enc_layout(q, src_len);
  uint8_t* slice = (uint8_t*)malloc(m.bytes);
  if (!slice) return 2;
  memset(slice, poison, m.bytes);
  lzenc::lzmaenc_init_slice(slice, m.l, 0, 1);
  uint32_t crc[256], prob_prices[lzenc::kProbPricesWords];
  for (uint32_t v = 0; v < 256; ++v) crc[v] = lzenc::crc_entry(v);
  for (uint32_t v = 0; v < lzenc::kProbPricesWords; ++v) prob_prices[v] = lzenc::prob_price_entry(v);
  lzenc::Out o;
  if (lzenc::mode_of(q) == 0) {
    lzenc::Lzma2Enc e;
    o = e.encode_block(src, uint32_t(src_len), dst, dst_cap, q, slice, m, crc);
  } else {
    lzenc::Lzma2EncNormal e;
    o = e.encode_block(src, uint32_t(src_len), dst, dst_cap, q, slice, m, crc, prob_prices);
  }
  free(slice);
  *dest_len = o.dest_len;
  return o.res;
}

// {LZMA slice bytes, LZMA2 slice bytes} of a mode
extern "C" void lzma2enc_opt_emu_slice_bytes(uint32_t dict_size, uint32_t lc, uint32_t lp,
                                             uint32_t pb, uint32_t algo, uint32_t bt,
                                             uint64_t src_len, uint64_t* out2) {
  lzenc::Params q{dict_size, lc, lp, pb, 5, 0, 0};
  q.algo = algo;
  q.bt = bt;
  out2[0] = lzenc::lzmaenc_layout(q, src_len).bytes;
  out2[1] = lzenc::lzma2enc_layout(q, src_len).bytes;
}

#ifdef LZMA2ENC_OPT_EMU_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned n = 0, bad = 0;
  for (;;) {
    int32_t h[6];
    uint64_t src_len, dst_cap, exp_dest;
    int32_t exp_res;
    if (fread(h, 4, 6, f) != 6) break;
    if (fread(&src_len, 8, 1, f) != 1 || fread(&dst_cap, 8, 1, f) != 1 ||
        fread(&exp_res, 4, 1, f) != 1 || fread(&exp_dest, 8, 1, f) != 1)
      return 2;
    // exact-size blocks: an over-read of the source or an over-write of the
    // destination is the sanitizer's to report
    uint8_t* src = (uint8_t*)malloc(src_len ? src_len : 1);
    uint8_t* want = (uint8_t*)malloc(exp_dest ? exp_dest : 1);
    if (fread(src, 1, src_len, f) != src_len || fread(want, 1, exp_dest, f) != exp_dest) return 2;
    for (int pass = 0; pass < 2; ++pass) {
      uint8_t* dst = (uint8_t*)malloc(dst_cap ? dst_cap : 1);
      uint8_t prop = 0;
      uint64_t dl = 0;
      const int res =
          lzma2enc_opt_emu_encode(src, src_len, dst, dst_cap, h[0], uint32_t(h[1]), h[2], h[3], h[4],
                                  uint32_t(h[5]), pass ? 0xA5 : 0x3C, &prop, &dl);
      if (res != exp_res || dl != exp_dest || memcmp(dst, want, exp_dest) != 0) {
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
