// pack_emu.cpp -- csrc/sevenz_pack_device.h on the host: the pack stage's four
// kernels run workgroup by workgroup, phase by phase, thread by thread, in the
// order the barriers of sevenzenc_kernels.hip allow.  Built as a shared library
// for tests/test_7zenc_host.py, or with -DSZPACK_EMU_MAIN as a stand-alone
// program (the sanitizer build) that runs a case file written by
// tests/sevenzpack_cases.py: exact-size 16-byte-aligned allocations, so a load
// outside the granules that hold a base's bytes is a sanitizer error.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sevenz_pack_device.h"

using szpack::kThreads;

extern "C" uint64_t szpack_emu_scratch_words(uint64_t n) { return szpack::scratch_words(n); }
extern "C" uint32_t szpack_emu_tile(void) { return kThreads; }

extern "C" void szpack_emu_run(const SzGpuPackArgs* args) {
  const SzGpuPackArgs a = *args;
  const uint64_t tiles = szpack::tiles_of(a.n);
  uint64_t sh[kThreads];
  *szpack::bad_of(a) = szpack::kNoBad;
  uint64_t* bad = szpack::bad_of(a);
  for (uint64_t b = 0; b < tiles; ++b) {  // collect
    for (uint32_t t = 0; t < kThreads; ++t)
      sh[t] = szpack::collect_item(a, b * kThreads + t, [bad](uint64_t k) {
        if (k < *bad) *bad = k;
      });
    szpack::collect_tile(a, b, sh);
  }
  {  // tiles
    uint64_t part[kThreads];
    for (uint32_t t = 0; t < kThreads; ++t) part[t] = szpack::tiles_part(a, t);
    szpack::tiles_total(a, part);
    for (uint32_t t = 0; t < kThreads; ++t) szpack::tiles_write(a, t, part[t]);
  }
  for (uint64_t b = 0; b < tiles; ++b) {  // offsets
    for (uint32_t t = 0; t < kThreads; ++t) {
      const uint64_t i = b * kThreads + t;
      sh[t] = i < a.n ? szpack::values_of(a)[i] : 0;
    }
    szpack::offsets_tile(a, b, sh);
    for (uint32_t t = 0; t < kThreads; ++t) szpack::offsets_item(a, b * kThreads + t, sh[t]);
  }
  if (a.d_total->res != szpack::kOk) return;  // gather
  // threads in descending order: no thread may depend on a lower one's stores
  for (uint64_t i = 0; i < a.n; ++i)
    for (uint32_t t = kThreads; t-- > 0;) szpack::gather_thread(a, i, t);
}

#ifdef SZPACK_EMU_MAIN
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

template <class T>
T* exact(size_t n) {  // whole 16-byte granules, nothing more
  const size_t bytes = (n * sizeof(T) + 15) & ~size_t(15);
  return static_cast<T*>(aligned_alloc(16, bytes ? bytes : 16));
}

}  // namespace

// File: u64 cases; per case: u64 n, n_folders, n_lzma, n_lzma2, n_ppmd, out_cap,
// out_mis, guard, base size[4] (~0 = NULL); pieces; the three result arrays;
// the bases' bytes; then what is expected: total (16 bytes), piece_off[n],
// u64 sizes_valid, folder_size[n_folders], the out image (out_cap + guard).
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  Reader r{fopen(argv[1], "rb")};
  if (!r.f) return 2;
  const uint64_t cases = r.u64();
  uint64_t bad = 0;
  for (uint64_t c = 0; c < cases && r.ok; ++c) {
    SzGpuPackArgs a;
    memset(&a, 0, sizeof(a));
    a.n = r.u64();
    a.n_folders = r.u64();
    a.n_lzma = r.u64();
    a.n_lzma2 = r.u64();
    a.n_ppmd = r.u64();
    a.out_cap = r.u64();
    const uint64_t out_mis = r.u64(), guard = r.u64();
    uint64_t bsize[LZMA_GPU_7Z_PACK_BASES];
    for (uint64_t& s : bsize) s = r.u64();
    SzGpuPackPiece* pieces = exact<SzGpuPackPiece>(a.n);
    LzmaEncGpuResult* lz = exact<LzmaEncGpuResult>(a.n_lzma);
    LzmaEncGpuResult* l2 = exact<LzmaEncGpuResult>(a.n_lzma2);
    Ppmd7GpuEncResult* pp = exact<Ppmd7GpuEncResult>(a.n_ppmd);
    r.get(pieces, a.n * sizeof(*pieces));
    r.get(lz, a.n_lzma * sizeof(*lz));
    r.get(l2, a.n_lzma2 * sizeof(*l2));
    r.get(pp, a.n_ppmd * sizeof(*pp));
    uint8_t* bases[LZMA_GPU_7Z_PACK_BASES];
    for (int k = 0; k < LZMA_GPU_7Z_PACK_BASES; ++k) {
      bases[k] = nullptr;
      if (bsize[k] == ~uint64_t(0)) continue;
      bases[k] = exact<uint8_t>(bsize[k]);
      r.get(bases[k], bsize[k]);
      a.bases[k] = bases[k];
    }
    const size_t image = size_t(a.out_cap + guard);
    uint8_t* out = exact<uint8_t>(out_mis + image);
    memset(out, 0xEE, out_mis + image);
    a.d_pieces = pieces;
    a.d_lzma = lz;
    a.d_lzma2 = l2;
    a.d_ppmd = pp;
    a.d_out = out + out_mis;
    a.d_scratch = exact<uint64_t>(szpack::scratch_words(a.n));
    a.d_piece_off = exact<uint64_t>(a.n);
    a.d_folder_size = exact<uint64_t>(a.n_folders);
    LzmaEncGpuResult total;
    a.d_total = &total;
    szpack_emu_run(&a);
    LzmaEncGpuResult want_total;
    r.get(&want_total, sizeof(want_total));
    std::vector<uint64_t> want_off(a.n), want_size(a.n_folders);
    std::vector<uint8_t> want_out(image);
    r.get(want_off.data(), a.n * 8);
    const uint64_t sizes_valid = r.u64();
    r.get(want_size.data(), a.n_folders * 8);
    r.get(want_out.data(), image);
    bool same = total.res == want_total.res && total._pad == want_total._pad &&
                total.dest_len == want_total.dest_len &&
                (a.n == 0 || memcmp(a.d_piece_off, want_off.data(), a.n * 8) == 0) &&
                (image == 0 || memcmp(a.d_out, want_out.data(), image) == 0);
    if (sizes_valid && a.n_folders)
      same = same && memcmp(a.d_folder_size, want_size.data(), a.n_folders * 8) == 0;
    for (uint64_t k = 0; k < out_mis; ++k) same = same && out[k] == 0xEE;
    if (!same) {
      ++bad;
      printf("case %llu differs\n", (unsigned long long)c);
    }
    free(pieces);
    free(lz);
    free(l2);
    free(pp);
    for (uint8_t* b : bases) free(b);
    free(out);
    free(a.d_scratch);
    free(a.d_piece_off);
    free(a.d_folder_size);
  }
  fclose(r.f);
  if (!r.ok) {
    printf("short case file\n");
    return 2;
  }
  printf("%llu cases, %llu mismatches\n", (unsigned long long)cases, (unsigned long long)bad);
  return bad ? 1 : 0;
}
#endif
