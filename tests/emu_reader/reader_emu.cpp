// TEST INFRASTRUCTURE ONLY (tests/test_reader_emu.py).
// A stand-alone program on the host build (-DLZGPU_HOST_EMU) of lzma_device.h,
// built with -fsanitize=address,undefined and run as a program:
//
//   reader_emu readers
//       GlobalReaderP and GlobalReaderQ against a plain byte cursor, for every
//       start alignment 0..15 and every avail 0..80.  The input lies in a heap
//       buffer that ends with the last 16-byte block holding a valid byte, so
//       a load of a block wholly outside [p, p + avail) is an ASan report.
//   reader_emu lanes JOB OUT
//       the lane emulation of the throughput placement over the streams of
//       JOB (written by the test: planned descriptors + inputs); result rows
//       and output bytes go to OUT.  The reader is a compile-time switch
//       (LZGPU_READER): the test builds the program once per reader and
//       compares the files.
#define LZGPU_HOST_EMU 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../lzma-sdk-zliblike_amd/csrc/lzma_lane.h"

using namespace lzgpu;

static uint64_t rng_state;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return uint32_t((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                     \
      fprintf(stderr, "\n");                            \
      exit(1);                                          \
    }                                                   \
  } while (0)

// the checkpoint hooks as the decoder calls them: GlobalReaderP's mid-walk
// checkpoint leaves its fetch to fetch_pending()
static void mid(GlobalReaderP& r) { r.topup_mid(); }
static void mid(GlobalReaderQ& r) { r.topup(); }
static void mid_end(GlobalReaderP& r) { r.fetch_pending(); }
static void mid_end(GlobalReaderQ&) {}

// One seeded sequence of reader calls that honours the checkpoint
// precondition (at most 5 take_u behind a checkpoint -- 4 where the window was
// empty before it --, advance / peek only on a non-empty window), every byte
// and every used() against the cursor.  The sequence goes on for `over` bytes past the input's end, where the bytes are
// unspecified but used() and the loads' bounds still hold.
template <class Rd>
static void drive(const uint8_t* p, uint32_t avail, uint64_t seed, uint32_t over, int al) {
  Rd rd;
  rd.init(p, avail);
  CHECK(rd.used() == 0, "used() after init: %u (align %d avail %u)", rd.used(), al, avail);
  if (avail == 0) return;
  rng_state = seed;
  uint32_t cur = 0;
  auto byte_ok = [&](uint32_t b) {
    if (cur < avail)
      CHECK(b == p[cur], "byte %u: %02x != %02x (align %d avail %u)", cur, b, p[cur], al, avail);
    ++cur;
    CHECK(rd.used() == cur, "used() %u != %u (align %d avail %u)", rd.used(), cur, al, avail);
  };
  while (cur < avail + over) {
    switch (rnd() % 5) {
      case 0:
      case 1: {  // a checkpoint, then up to 5 unchecked bytes
        const uint32_t had = rd.nb;
        rd.topup();
        CHECK(rd.nb >= (had ? 5u : 4u), "topup: %u -> %u bytes", had, rd.nb);
        for (uint32_t k = rnd() % 6; k != 0 && rd.nb != 0; --k) byte_ok(rd.take_u());
        break;
      }
      case 2: {  // the literal's mid-walk checkpoint: unchecked bytes, then the fetch
        rd.topup();
        for (uint32_t k = rnd() % 5; k != 0 && rd.nb > 1; --k) byte_ok(rd.take_u());
        mid(rd);
        CHECK(rd.nb >= 5, "mid-walk topup left %u bytes", rd.nb);
        for (uint32_t k = rnd() % 5; k != 0; --k) byte_ok(rd.take_u());
        mid_end(rd);
        break;
      }
      case 3:
        byte_ok(rd.next());
        break;
      default:
        if (rd.nb != 0) {
          const bool n = (rnd() & 1) != 0;
          const uint32_t b = rd.peek();
          rd.advance(n);
          if (n) byte_ok(b);
        }
        break;
    }
  }
}

static int run_readers() {
  for (int al = 0; al < 16; ++al) {
    for (uint32_t avail = 0; avail <= 80; ++avail) {
      // blocks from p's 16-byte block through the last one with a valid byte
      const size_t blocks = avail ? (size_t(al) + avail + 15) / 16 : 0;
      // (avail 0: no block may be loaded, so p's own block lies behind the end
      // of a 16-byte allocation)
      uint8_t* buf = (uint8_t*)aligned_alloc(16, blocks ? blocks * 16 : 16);
      CHECK(buf != nullptr, "aligned_alloc");
      const uint8_t* p = (const uint8_t*)(uintptr_t(buf) + (blocks ? 0 : 16) + uintptr_t(al));
      rng_state = 0x9E3779B97F4A7C15ull + uint64_t(al) * 131 + avail;
      for (size_t i = 0; i < (blocks ? blocks * 16 : 16); ++i) buf[i] = uint8_t(rnd() >> 7);
      for (uint64_t seed = 1; seed <= 6; ++seed) {
        const uint64_t sd = seed * 0x100000001B3ull + uint64_t(al) * 977 + avail;
        drive<GlobalReaderP>(p, avail, sd, 24, al);
        drive<GlobalReaderQ>(p, avail, sd, 24, al);
      }
      free(buf);
    }
  }
  printf("readers ok\n");
  return 0;
}

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

// JOB: u64 n, src bytes, dst bytes, workspace bytes, LDS stride (cells); n
// descriptors; the inputs.  OUT: n result rows, the output buffer.
static int run_lanes(const char* job_path, const char* out_path) {
  const std::vector<uint8_t> job = read_file(job_path);
  CHECK(job.size() >= 40, "short job");
  uint64_t h[5];
  memcpy(h, job.data(), sizeof h);
  const size_t n = h[0], src_bytes = h[1], dst_bytes = h[2], ws_bytes = h[3];
  const uint32_t stride = uint32_t(h[4]);
  CHECK(job.size() == 40 + n * sizeof(LzmaGpuStreamDesc) + src_bytes, "job size");
  std::vector<LzmaGpuStreamDesc> descs(n);
  memcpy(descs.data(), job.data() + 40, n * sizeof(LzmaGpuStreamDesc));
  // the inputs in a 16-byte aligned buffer of their own that ends with the
  // last 16-byte block holding an input byte
  const size_t src_alloc = ((src_bytes + 15) & ~size_t(15)) + (src_bytes ? 0 : 16);
  uint8_t* src = (uint8_t*)aligned_alloc(16, src_alloc);
  CHECK(src != nullptr, "aligned_alloc");
  memset(src, 0xC3, src_alloc);
  memcpy(src, job.data() + 40 + n * sizeof(LzmaGpuStreamDesc), src_bytes);
  std::vector<uint8_t> dst(dst_bytes + 1, 0xEE);
  std::vector<uint16_t> ws(ws_bytes / 2 + 8);
  std::vector<uint16_t> slab(stride + 8);
  std::vector<LzmaGpuResult> res(n);
  for (size_t i = 0; i < n; ++i) {
    memset(slab.data(), 0xA5, slab.size() * 2);  // LDS is not zeroed between workgroups
    memset(&res[i], 0, sizeof res[i]);
    res[i] = lane_decode_lds(descs[i], src, dst.data(), ws.data(), slab.data(), stride);
  }
  FILE* f = fopen(out_path, "wb");
  CHECK(f != nullptr, "open %s", out_path);
  for (size_t i = 0; i < n; ++i) {
    const int64_t row[4] = {res[i].res, res[i].status, int64_t(res[i].dest_len),
                            int64_t(res[i].src_len)};
    fwrite(row, sizeof row, 1, f);
  }
  fwrite(dst.data(), 1, dst_bytes, f);
  fclose(f);
  free(src);
  printf("lanes ok: %zu streams, reader %d\n", n, int(LZGPU_READER));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && strcmp(argv[1], "readers") == 0) return run_readers();
  if (argc == 4 && strcmp(argv[1], "lanes") == 0) return run_lanes(argv[2], argv[3]);
  fprintf(stderr, "usage: reader_emu readers | reader_emu lanes JOB OUT\n");
  return 2;
}
