// Host build of csrc/ppmd7_device.h's encoder: what ppmd7_encode_kernel runs, as
// lane 0 of 1.
//   shared library: ppmd7_emu_encode() for tests/test_ppmd7enc_emu.py (ctypes)
//   -DPPMD7ENC_EMU_MAIN: a stand-alone program over a case file, for sanitizer runs:
//     records of  u32 order, u32 mem_size, u64 src_len, u64 dst_cap, i32 res,
//     u64 dest_len, u64 packed_len, then src_len plain bytes and dest_len expected bytes
#define PPMD7_HOST_EMU 1
#include <stdint.h>

// counters[0] bytes-out events with a carry, [1] with 0xFF bytes pending behind
// the held byte (CacheSize > 1), [2] with both: a carry rippling through a run
static uint64_t g_count[3];
#define PPMD7_ENC_COUNT(carry, pending) \
  (g_count[0] += (carry) != 0, g_count[1] += (pending) > 1, g_count[2] += (carry) != 0 && (pending) > 1)
#include "ppmd7_device.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" int ppmd7_emu_encode(const uint8_t* src, uint64_t src_len, uint8_t* dst,
                                uint64_t dst_cap, uint32_t order, uint32_t mem_size,
                                uint64_t* dest_len, uint64_t* packed_len, uint64_t* counters) {
  // exact-size heap blocks, so that a sanitizer sees any access outside them
  uint8_t* model = nullptr;
  if (mem_size >= kPpmd7MinMem && mem_size <= kPpmd7MaxMem)
    model = (uint8_t*)aligned_alloc(4, (ppmd7_model_bytes(mem_size) + 3) & ~uint64_t(3));
  Ppmd7Hot* hot = new Ppmd7Hot;
  uint16_t* bin = new uint16_t[kPpmd7BinCells];
  Ppmd7 t;
  t.h = hot;
  t.build_tables();
  g_count[0] = g_count[1] = g_count[2] = 0;
  const Ppmd7EncOut r =
      ppmd7_encode_stream(src, src_len, dst, dst_cap, order, mem_size, model, hot, bin, 0, 1);
  delete hot;
  delete[] bin;
  free(model);
  *dest_len = r.dest_len;
  *packed_len = r.packed_len;
  if (counters) memcpy(counters, g_count, sizeof(g_count));
  return r.res;
}

#ifdef PPMD7ENC_EMU_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned n = 0, bad = 0;
  for (;;) {
    uint32_t order, mem;
    uint64_t src_len, dst_cap, exp_dest, exp_packed;
    int32_t exp_res;
    if (fread(&order, 4, 1, f) != 1) break;
    if (fread(&mem, 4, 1, f) != 1 || fread(&src_len, 8, 1, f) != 1 ||
        fread(&dst_cap, 8, 1, f) != 1 || fread(&exp_res, 4, 1, f) != 1 ||
        fread(&exp_dest, 8, 1, f) != 1 || fread(&exp_packed, 8, 1, f) != 1)
      return 2;
    // exact-size copies: an over-read of the input or an over-write of the
    // output is the sanitizer's to report
    uint8_t* src = (uint8_t*)malloc(src_len ? src_len : 1);
    uint8_t* want = (uint8_t*)malloc(exp_dest ? exp_dest : 1);
    uint8_t* dst = (uint8_t*)malloc(dst_cap ? dst_cap : 1);
    if (fread(src, 1, src_len, f) != src_len || fread(want, 1, exp_dest, f) != exp_dest) return 2;
    uint64_t dl = 0, pl = 0;
    const int res = ppmd7_emu_encode(src, src_len, dst, dst_cap, order, mem, &dl, &pl, nullptr);
    if (res != exp_res || dl != exp_dest || pl != exp_packed || memcmp(dst, want, exp_dest) != 0) {
      printf("case %u: got (%d, %llu, %llu) want (%d, %llu, %llu)\n", n, res,
             (unsigned long long)dl, (unsigned long long)pl, exp_res,
             (unsigned long long)exp_dest, (unsigned long long)exp_packed);
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
