// Host build of csrc/ppmd7_device.h: the decoder the kernel runs, as lane 0 of 1.
//   shared library: ppmd7_emu_decode() for tests/test_ppmd7_emu.py (ctypes)
//   -DPPMD7_EMU_MAIN: a stand-alone program over a case file, for sanitizer runs:
//     records of  u32 order, u32 mem_size, u64 src_len, u64 dst_len, i32 res,
//     u64 dest_len, u64 src_used, then src_len packed bytes and dest_len expected bytes
#define PPMD7_HOST_EMU 1
#include "ppmd7_device.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

extern "C" int ppmd7_emu_decode(const uint8_t* src, uint64_t src_len, uint8_t* dst,
                                uint64_t dst_len, uint32_t order, uint32_t mem_size,
                                uint64_t* dest_len, uint64_t* src_used) {
  // exact-size heap blocks, so that a sanitizer sees any access outside them
  std::vector<uint32_t> model;
  if (mem_size >= kPpmd7MinMem && mem_size <= kPpmd7MaxMem)
    model.resize((ppmd7_model_bytes(mem_size) + 3) / 4);
  Ppmd7Hot* hot = new Ppmd7Hot;
  uint16_t* bin = new uint16_t[kPpmd7BinCells];
  Ppmd7 t;
  t.h = hot;
  t.build_tables();
  const Ppmd7Out r = ppmd7_decode_stream(src, src_len, dst, dst_len, order, mem_size,
                                         (uint8_t*)model.data(), hot, bin, 0, 1);
  delete hot;
  delete[] bin;
  *dest_len = r.dest_len;
  *src_used = r.src_len;
  return r.res;
}

#ifdef PPMD7_EMU_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned n = 0, bad = 0;
  for (;;) {
    uint32_t order, mem;
    uint64_t src_len, dst_len, exp_dest, exp_src;
    int32_t exp_res;
    if (fread(&order, 4, 1, f) != 1) break;
    if (fread(&mem, 4, 1, f) != 1 || fread(&src_len, 8, 1, f) != 1 ||
        fread(&dst_len, 8, 1, f) != 1 || fread(&exp_res, 4, 1, f) != 1 ||
        fread(&exp_dest, 8, 1, f) != 1 || fread(&exp_src, 8, 1, f) != 1)
      return 2;
    // exact-size copies: an over-read of the input or an over-write of the
    // output is the sanitizer's to report
    uint8_t* src = (uint8_t*)malloc(src_len ? src_len : 1);
    uint8_t* want = (uint8_t*)malloc(exp_dest ? exp_dest : 1);
    uint8_t* dst = (uint8_t*)malloc(dst_len ? dst_len : 1);
    if (fread(src, 1, src_len, f) != src_len || fread(want, 1, exp_dest, f) != exp_dest) return 2;
    uint64_t dl = 0, sl = 0;
    const int res = ppmd7_emu_decode(src, src_len, dst, dst_len, order, mem, &dl, &sl);
    if (res != exp_res || dl != exp_dest || sl != exp_src || memcmp(dst, want, exp_dest) != 0) {
      printf("case %u: got (%d, %llu, %llu) want (%d, %llu, %llu)\n", n, res,
             (unsigned long long)dl, (unsigned long long)sl, exp_res,
             (unsigned long long)exp_dest, (unsigned long long)exp_src);
      ++bad;
    }
    free(src);
    free(want);
    free(dst);
    ++n;
  }
  fclose(f);
  printf("%u cases, %u mismatches\n", n, bad);
  return bad ? 1 : 0;
}
#endif
