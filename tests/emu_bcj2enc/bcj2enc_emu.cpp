// bcj2enc_emu.cpp -- csrc/bcj2enc_device.h on the host: the five launches of
// bcj2enc_kernels.hip run workgroup by workgroup, phase by phase, thread by
// thread, in the order their barriers allow (threads in descending order where
// none may depend on a lower one).  Built as a shared library for
// tests/test_bcj2enc_emu.py, or with -DBCJ2ENC_EMU_MAIN as a stand-alone program
// (the sanitizer build) that runs a case file written by tests/bcj2enc_cases.py:
// exact-size allocations for the source, the scratch and the descriptors, so a
// read outside a stream's bytes is a sanitizer error.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bcj2enc_device.h"

using namespace bcj2enc;

extern "C" uint64_t bcj2enc_emu_scratch(const Bcj2GpuEncDesc* descs, uint64_t n) {
  uint64_t bytes = fixed_bytes();
  for (uint64_t i = 0; i < n; ++i) bytes += slice_bytes(descs[i].src_len);
  return bytes;
}
// run, segment and workgroup step in bytes: the boundaries the cases straddle
extern "C" void bcj2enc_emu_geometry(uint32_t out[3]) {
  out[0] = kRun;
  out[1] = kSeg;
  out[2] = kSeg * kWaves;
}

static void scan(Elem buf[2][kWave]) {
  for (uint32_t k = 0; k < kScanSteps; ++k)
    for (uint32_t lane = kWave; lane-- > 0;) scan_step(buf[k & 1], buf[(k + 1) & 1], lane, k);
}

// grid: the workgroups of the classify and scatter launches (any value >= 1
// gives the same bytes)
extern "C" void bcj2enc_emu_run(const Bcj2GpuEncDesc* descs, uint64_t n, const uint8_t* src,
                                uint8_t* dst, uint8_t* scratch, Bcj2GpuEncResult* results,
                                uint32_t grid) {
  if (n == 0) return;
  Args a;
  a.descs = descs;
  a.n = n;
  a.src = src;
  a.dst = dst;
  a.scratch = scratch;
  a.results = results;
  {  // plan
    std::vector<uint64_t> segs(kThreads), bytes(kThreads);
    for (uint32_t t = 0; t < kThreads; ++t) plan_part(a, t, &segs[t], &bytes[t]);
    plan_total(a, segs.data(), bytes.data());
    for (uint32_t t = kThreads; t-- > 0;) plan_write(a, t, segs[t], bytes[t]);
  }
  const uint64_t total = header_of(a)->segs;
  static Elem sh[kWaves][2][kWave];
  for (int pass = 0; pass < 2; ++pass) {  // classify, then streams, then scatter
    for (uint32_t block = 0; block < grid; ++block)
      for (uint64_t first = uint64_t(block) * kWaves; first < total;
           first += uint64_t(grid) * kWaves)
        for (uint32_t wave = 0; wave < kWaves; ++wave) {
          const SegRef r = seg_ref(a, first + wave);
          for (uint32_t lane = 0; lane < kWave; ++lane) sh[wave][0][lane] = seg_elem(a, r, lane, src);
          scan(sh[wave]);
          if (pass == 0)
            classify_put(a, r, sh[wave][kScanOut][kWave - 1]);
          else
            for (uint32_t lane = kWave; lane-- > 0;)
              scatter_thread(a, r, lane, sh[wave][kScanOut], src, dst);
        }
    if (pass == 1) break;
    for (uint64_t stream = 0; stream < n; ++stream) {  // streams
      static Elem maps[2][kWave], sums[2][kWave];
      const uint64_t segs = segs_of(descs[stream].src_len);
      uint32_t carry = 0, tot[3] = {0, 0, 0};
      for (uint64_t first = 0; first < segs; first += kWave) {
        Elem own[kWave];
        for (uint32_t lane = 0; lane < kWave; ++lane) maps[0][lane] = streams_map(a, stream, first, lane);
        scan(maps);
        for (uint32_t lane = 0; lane < kWave; ++lane)
          sums[0][lane] = own[lane] = streams_counts(a, stream, first, lane, maps[kScanOut], carry);
        for (uint32_t k = 0; k < kScanSteps; ++k)
          for (uint32_t lane = kWave; lane-- > 0;) add_step(sums[k & 1], sums[(k + 1) & 1], lane, k);
        for (uint32_t lane = 0; lane < kWave; ++lane)
          streams_put(a, stream, first, lane, own[lane], sums[kScanOut], tot);
        streams_next(maps[kScanOut], sums[kScanOut], &carry, tot);
      }
      streams_total(a, stream, tot);
    }
  }
  for (uint64_t stream = 0; stream < n; ++stream) {  // code
    uint16_t prob[258];
    code_stream(a, stream, dst, prob);
  }
}

#ifdef BCJ2ENC_EMU_MAIN
namespace {

struct Reader {
  FILE* f;
  bool ok = true;
  void get(void* p, size_t n) {
    if (n && fread(p, 1, n, f) != n) ok = false;
  }
  uint64_t u64() {
    uint64_t v = 0;
    get(&v, 8);
    return v;
  }
};

}  // namespace

// File: u64 batches; per batch: u64 n, dst_size, grid; the n descriptors; per
// stream its source bytes (src_off = the running sum: the source buffer is
// exactly the streams); then what is expected: the n results and the dst image
// (dst_size bytes, 0xEE where nothing is written).
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Reader r{fopen(argv[1], "rb")};
  if (!r.f) return 2;
  const uint64_t batches = r.u64();
  uint64_t bad = 0, streams = 0;
  for (uint64_t c = 0; c < batches && r.ok; ++c) {
    const uint64_t n = r.u64(), dst_size = r.u64(), grid = r.u64();
    Bcj2GpuEncDesc* descs = static_cast<Bcj2GpuEncDesc*>(malloc(n ? n * sizeof(Bcj2GpuEncDesc) : 1));
    r.get(descs, n * sizeof(Bcj2GpuEncDesc));
    uint64_t src_size = 0;
    for (uint64_t i = 0; i < n && r.ok; ++i) src_size += descs[i].src_len;
    if (!r.ok) break;
    uint8_t* src = static_cast<uint8_t*>(malloc(src_size ? src_size : 1));
    r.get(src, src_size);
    uint8_t* dst = static_cast<uint8_t*>(malloc(dst_size ? dst_size : 1));
    memset(dst, 0xEE, dst_size);
    const uint64_t sbytes = bcj2enc_emu_scratch(descs, n);
    uint8_t* scratch = static_cast<uint8_t*>(aligned_alloc(16, (sbytes + 15) & ~uint64_t(15)));
    memset(scratch, 0xA7, sbytes);
    std::vector<Bcj2GpuEncResult> got(n), want(n);
    std::vector<uint8_t> image(dst_size);
    bcj2enc_emu_run(descs, n, src, dst, scratch, got.data(), uint32_t(grid));
    r.get(want.data(), n * sizeof(Bcj2GpuEncResult));
    r.get(image.data(), dst_size);
    bool same = dst_size == 0 || memcmp(dst, image.data(), dst_size) == 0;
    for (uint64_t i = 0; i < n; ++i) {
      same = same && got[i].res == want[i].res;
      for (int k = 0; k < 4; ++k) same = same && got[i].len[k] == want[i].len[k];
    }
    if (!same) {
      ++bad;
      printf("batch %llu differs\n", (unsigned long long)c);
    }
    streams += n;
    free(descs);
    free(src);
    free(dst);
    free(scratch);
  }
  fclose(r.f);
  if (!r.ok) {
    printf("short case file\n");
    return 2;
  }
  printf("%llu batches, %llu streams, %llu mismatches\n", (unsigned long long)batches,
         (unsigned long long)streams, (unsigned long long)bad);
  return bad ? 1 : 0;
}
#endif
