// sevenz_pack_device.h -- the pack stage of the 7z writer: the finished pieces
// of an archive's encode batches (LZMA streams, LZMA2 blocks, PPMd7 streams,
// Copy ranges of the source) gathered into the archive's pack area, on the
// device.  Shared by sevenzenc_kernels.hip (the kernels are thin wrappers: one
// call per thread and phase, a barrier between phases) and by the host
// emulator (tests/emu_7zpack/), which runs the same phases thread by thread.
//
//   collect   piece i's value = its length (the result's dest_len of its kind,
//             or the Copy range's own) + 1 for the 0x00 that ends an LZMA2
//             folder; the first piece that failed; one sum per tile of
//             kThreads pieces
//   tiles     one workgroup: exclusive scan of the tile sums (a serial run per
//             thread, then one serial pass over the kThreads partial sums), the
//             total and the verdict
//   offsets   per tile: exclusive scan of its values from the tile's base =
//             every piece's place in the pack area; a folder's first piece
//             leaves the folder's start
//   gather    one workgroup per piece: 16-byte stores aligned to the
//             destination, each made from two aligned 16-byte loads (both in
//             granules that hold bytes of the piece), head and tail by bytes;
//             the 0x00 after an LZMA2 folder; a folder's last piece turns the
//             folder's start into its pack size.  Nothing is written when a
//             piece failed or the total exceeds the capacity.
//
// Scratch (uint64): values[n] | tile sums[tiles] | first failed piece[1].
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/lzma_gpu.h"

#if defined(__HIPCC__)
#define SZPACK_FN __host__ __device__ inline
#else
#define SZPACK_FN inline
#endif

namespace szpack {

constexpr uint32_t kThreads = 256;  // threads of a workgroup = pieces of a tile
constexpr int32_t kOk = 0, kErrParam = 5, kErrOutputEof = 7;
constexpr uint64_t kNoBad = ~uint64_t(0);

SZPACK_FN uint64_t tiles_of(uint64_t n) { return (n + kThreads - 1) / kThreads; }
SZPACK_FN uint64_t scratch_words(uint64_t n) { return n + tiles_of(n) + 1; }
SZPACK_FN uint64_t* values_of(const SzGpuPackArgs& a) { return a.d_scratch; }
SZPACK_FN uint64_t* tile_sums_of(const SzGpuPackArgs& a) { return a.d_scratch + a.n; }
SZPACK_FN uint64_t* bad_of(const SzGpuPackArgs& a) { return a.d_scratch + a.n + tiles_of(a.n); }

struct Val {
  uint64_t len;  // the piece's bytes
  int32_t res;   // kOk, the encoder's verdict, or kErrParam for an entry out of range
};

// Reads nothing outside the tables: an index out of range is kErrParam.
SZPACK_FN Val piece_value(const SzGpuPackArgs& a, uint64_t i) {
  const SzGpuPackPiece p = a.d_pieces[i];
  Val v;
  v.len = 0;
  v.res = kErrParam;
  if (p.folder >= a.n_folders || p.base >= LZMA_GPU_7Z_PACK_BASES || !a.bases[p.base] ||
      (p.flags & ~uint32_t(LZMA_GPU_7Z_PACK_LAST)))
    return v;
  switch (p.kind) {
    case LZMA_GPU_7Z_PACK_COPY:
      v.len = p.len;
      v.res = kOk;
      break;
    case LZMA_GPU_7Z_PACK_LZMA:
      if (p.slot >= a.n_lzma) return v;
      v.res = a.d_lzma[p.slot].res;
      v.len = a.d_lzma[p.slot].dest_len;
      break;
    case LZMA_GPU_7Z_PACK_LZMA2:
      if (p.slot >= a.n_lzma2) return v;
      v.res = a.d_lzma2[p.slot].res;
      v.len = a.d_lzma2[p.slot].dest_len;
      break;
    case LZMA_GPU_7Z_PACK_PPMD:
      if (p.slot >= a.n_ppmd) return v;
      v.res = a.d_ppmd[p.slot].res;
      v.len = a.d_ppmd[p.slot].dest_len;
      break;
    default:
      return v;
  }
  if (v.res != kOk) v.len = 0;
  return v;
}

// collect, every thread: the value of piece i (0 past the end), stored; `fail`
// is called with the index of a piece that is not kOk (the kernel's atomicMin)
template <class Fail>
SZPACK_FN uint64_t collect_item(const SzGpuPackArgs& a, uint64_t i, Fail fail) {
  if (i >= a.n) return 0;
  const Val v = piece_value(a, i);
  if (v.res != kOk) fail(i);
  const uint64_t val = v.len + ((a.d_pieces[i].flags & LZMA_GPU_7Z_PACK_LAST) ? 1u : 0u);
  values_of(a)[i] = val;
  return val;
}
// collect, thread 0 after the barrier: the tile's sum
SZPACK_FN void collect_tile(const SzGpuPackArgs& a, uint64_t tile, const uint64_t* sh) {
  uint64_t sum = 0;
  for (uint32_t j = 0; j < kThreads; ++j) sum += sh[j];
  tile_sums_of(a)[tile] = sum;
}

// tiles, every thread: the sum of its run of tile sums
SZPACK_FN void tiles_run(const SzGpuPackArgs& a, uint32_t t, uint64_t* lo, uint64_t* hi) {
  const uint64_t tiles = tiles_of(a.n);
  const uint64_t per = (tiles + kThreads - 1) / kThreads;
  *lo = uint64_t(t) * per < tiles ? uint64_t(t) * per : tiles;
  *hi = *lo + per < tiles ? *lo + per : tiles;
}
SZPACK_FN uint64_t tiles_part(const SzGpuPackArgs& a, uint32_t t) {
  uint64_t lo, hi, sum = 0;
  tiles_run(a, t, &lo, &hi);
  for (uint64_t k = lo; k < hi; ++k) sum += tile_sums_of(a)[k];
  return sum;
}
// tiles, thread 0 after the barrier: part[] becomes exclusive; the total
SZPACK_FN void tiles_total(const SzGpuPackArgs& a, uint64_t* part) {
  uint64_t run = 0;
  for (uint32_t j = 0; j < kThreads; ++j) {
    const uint64_t v = part[j];
    part[j] = run;
    run += v;
  }
  const uint64_t bad = *bad_of(a);
  LzmaEncGpuResult r;
  r._pad = 0;
  if (bad != kNoBad && bad < a.n) {
    r.res = piece_value(a, bad).res;
    if (r.res == kOk) r.res = kErrParam;
    r._pad = uint32_t(bad);
  } else {
    r.res = run > a.out_cap ? kErrOutputEof : kOk;
  }
  r.dest_len = run;
  *a.d_total = r;
}
// tiles, every thread after the second barrier: the tile sums become tile bases
SZPACK_FN void tiles_write(const SzGpuPackArgs& a, uint32_t t, uint64_t at) {
  uint64_t lo, hi;
  tiles_run(a, t, &lo, &hi);
  for (uint64_t k = lo; k < hi; ++k) {
    const uint64_t v = tile_sums_of(a)[k];
    tile_sums_of(a)[k] = at;
    at += v;
  }
}

// offsets, thread 0 after the barrier: sh[] (the tile's values) becomes the
// pieces' offsets
SZPACK_FN void offsets_tile(const SzGpuPackArgs& a, uint64_t tile, uint64_t* sh) {
  uint64_t run = tile_sums_of(a)[tile];
  for (uint32_t j = 0; j < kThreads; ++j) {
    const uint64_t v = sh[j];
    sh[j] = run;
    run += v;
  }
}
// offsets, every thread after the second barrier
SZPACK_FN void offsets_item(const SzGpuPackArgs& a, uint64_t i, uint64_t off) {
  if (i >= a.n) return;
  a.d_piece_off[i] = off;
  const uint32_t f = a.d_pieces[i].folder;
  if (f < a.n_folders && (i == 0 || a.d_pieces[i - 1].folder != f)) a.d_folder_size[f] = off;
}

struct V16 {
  uint32_t x, y, z, w;
};
SZPACK_FN V16 load16(const uint8_t* p) {  // p 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  return V16{v.x, v.y, v.z, v.w};
#else
  V16 v;
  memcpy(&v, p, 16);
  return v;
#endif
}
SZPACK_FN void store16(uint8_t* p, V16 v) {  // p 16-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<uint4*>(p) = make_uint4(v.x, v.y, v.z, v.w);
#else
  memcpy(p, &v, 16);
#endif
}
SZPACK_FN uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t bits) {
  return uint32_t(((uint64_t(hi) << 32) | lo) >> bits);
}

// thread t of kThreads moves its share of len bytes from s to d (any alignment)
SZPACK_FN void move_bytes(const uint8_t* s, uint8_t* d, uint64_t len, uint32_t t) {
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
  if (head > len) head = len;
  const uint64_t vecs = (len - head) >> 4;
  const uint64_t tail_at = head + (vecs << 4);
  for (uint64_t i = t; i < head; i += kThreads) d[i] = s[i];
  for (uint64_t i = tail_at + t; i < len; i += kThreads) d[i] = s[i];
  if (vecs == 0) return;
  // d + head is 16-byte aligned; s + head is `sh` bytes into an aligned 16
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s + head);
  const uint32_t sh = uint32_t(sa & 15);
  const uint8_t* sv = s + head - sh;
  uint8_t* dv = d + head;
  if (sh == 0) {
    for (uint64_t i = t; i < vecs; i += kThreads) store16(dv + (i << 4), load16(sv + (i << 4)));
    return;
  }
  // the second load's 16 bytes hold the vector's last source byte, so both
  // loads stay inside aligned 16-byte granules that hold bytes of the piece
  const uint32_t word = sh >> 2, bits = (sh & 3) * 8;
  for (uint64_t i = t; i < vecs; i += kThreads) {
    const V16 a = load16(sv + (i << 4)), c = load16(sv + (i << 4) + 16);
    V16 v;
    switch (word) {  // uniform over the workgroup
      case 0:
        v = V16{funnel(a.x, a.y, bits), funnel(a.y, a.z, bits), funnel(a.z, a.w, bits),
                funnel(a.w, c.x, bits)};
        break;
      case 1:
        v = V16{funnel(a.y, a.z, bits), funnel(a.z, a.w, bits), funnel(a.w, c.x, bits),
                funnel(c.x, c.y, bits)};
        break;
      case 2:
        v = V16{funnel(a.z, a.w, bits), funnel(a.w, c.x, bits), funnel(c.x, c.y, bits),
                funnel(c.y, c.z, bits)};
        break;
      default:
        v = V16{funnel(a.w, c.x, bits), funnel(c.x, c.y, bits), funnel(c.y, c.z, bits),
                funnel(c.z, c.w, bits)};
        break;
    }
    store16(dv + (i << 4), v);
  }
}

// gather, thread t of the workgroup that has piece i.  The caller has checked
// d_total->res == kOk, so every value is a finished piece's and the total fits
// out_cap.
SZPACK_FN void gather_thread(const SzGpuPackArgs& a, uint64_t i, uint32_t t) {
  const SzGpuPackPiece p = a.d_pieces[i];
  const uint64_t off = a.d_piece_off[i];
  const uint64_t val = values_of(a)[i];
  const bool last = (p.flags & LZMA_GPU_7Z_PACK_LAST) != 0;
  const uint64_t len = val - (last ? 1u : 0u);
  move_bytes(a.bases[p.base] + p.off, a.d_out + off, len, t);
  if (t != 0) return;
  if (last) a.d_out[off + len] = 0;
  if (i + 1 == a.n || a.d_pieces[i + 1].folder != p.folder)
    a.d_folder_size[p.folder] = off + val - a.d_folder_size[p.folder];
}

}  // namespace szpack
