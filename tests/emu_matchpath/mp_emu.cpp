// TEST INFRASTRUCTURE ONLY (tests/test_matchpath_emu.py).
// A stand-alone program on the host build (-DLZGPU_HOST_EMU) of lzma_device.h,
// built with -fsanitize=address,undefined and run as a program:
//
//   mp_emu JOB OUT
//       the lane emulation of the throughput placement (-DEMU_ILV: with
//       lane-interleaved global rows) over the streams of JOB; result rows and
//       output bytes go to OUT.  The match path's load batches are a
//       compile-time switch (LZGPU_MP): the test builds the program per value.
//
// JOB: u64 n, src bytes, dst bytes, workspace bytes, LDS stride (cells); n
// descriptors; the inputs.  OUT: n rows of four i64, the output buffer.
// Every buffer has its exact size on the heap: a batch load that leaves the
// lane's table, its rows or the input is an AddressSanitizer report.
#define LZGPU_HOST_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../lzma-sdk-zliblike_amd/csrc/lzma_lane.h"

using namespace lzgpu;

#define CHECK(c, ...)                                      \
  do {                                                     \
    if (!(c)) {                                            \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      exit(1);                                             \
    }                                                      \
  } while (0)

static std::vector<uint8_t> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f != nullptr, "open %s", path);
  std::vector<uint8_t> v;
  uint8_t tmp[65536];
  size_t n;
  while ((n = fread(tmp, 1, sizeof tmp, f)) != 0) v.insert(v.end(), tmp, tmp + n);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: mp_emu JOB OUT\n");
    return 2;
  }
  const std::vector<uint8_t> job = read_file(argv[1]);
  CHECK(job.size() >= 40, "short job");
  uint64_t h[5];
  memcpy(h, job.data(), sizeof h);
  const size_t n = h[0], src_bytes = h[1], dst_bytes = h[2], ws_bytes = h[3];
  const uint32_t stride = uint32_t(h[4]);
  CHECK(job.size() == 40 + n * sizeof(LzmaGpuStreamDesc) + src_bytes, "job size");
  std::vector<LzmaGpuStreamDesc> descs(n);
  memcpy(descs.data(), job.data() + 40, n * sizeof(LzmaGpuStreamDesc));
  // the inputs in a 16-byte aligned buffer that ends with the last 16-byte
  // block holding an input byte
  const size_t src_alloc = ((src_bytes + 15) & ~size_t(15)) + (src_bytes ? 0 : 16);
  uint8_t* src = (uint8_t*)aligned_alloc(16, src_alloc);
  CHECK(src != nullptr, "aligned_alloc");
  memset(src, 0xC3, src_alloc);
  memcpy(src, job.data() + 40 + n * sizeof(LzmaGpuStreamDesc), src_bytes);
  std::vector<uint8_t> dst(dst_bytes + 1, 0xEE);
  std::vector<uint16_t> ws(ws_bytes / 2 + 8);
  std::vector<uint16_t> slab(stride);
  std::vector<LzmaGpuResult> res(n);
#if defined(EMU_ILV)
  // 32 lane columns of exactly the widest stream's global rows; stream i runs
  // in column i % 32 beside its neighbours' stale cells
  size_t rows = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t lc, lp, pb, dict;
    if (lz_props_parse(descs[i].props, 5, lc, lp, pb, dict) != kOk) continue;
    const size_t r = make_layout(lc, lp, pb, LZGPU_LDS_MASK).glb_cells;
    rows = r > rows ? r : rows;
  }
  std::vector<uint16_t> slots(rows * kIlv, 0x5A5A);
#endif
  for (size_t i = 0; i < n; ++i) {
    memset(slab.data(), 0xA5, slab.size() * 2);  // LDS is not zeroed between workgroups
    memset(&res[i], 0, sizeof res[i]);
#if defined(EMU_ILV)
    res[i] = lane_decode_lds<LZGPU_LDS_MASK | kIlvBit>(descs[i], src, dst.data(), ws.data(),
                                                      slab.data(), stride,
                                                      slots.data() + (i % kIlv) * kIlvLaneCells);
#else
    res[i] = lane_decode_lds(descs[i], src, dst.data(), ws.data(), slab.data(), stride);
#endif
  }
  FILE* f = fopen(argv[2], "wb");
  CHECK(f != nullptr, "open %s", argv[2]);
  for (size_t i = 0; i < n; ++i) {
    const int64_t row[4] = {res[i].res, res[i].status, int64_t(res[i].dest_len),
                            int64_t(res[i].src_len)};
    fwrite(row, sizeof row, 1, f);
  }
  fwrite(dst.data(), 1, dst_bytes, f);
  fclose(f);
  free(src);
  printf("lanes ok: %zu streams, LZGPU_MP %d\n", n, int(LZGPU_MP));
  return 0;
}
