// xz_capi.hip -- the xz container: its index (LzmaGpu_XzIndex) and the block
// batch (LzmaGpu_XzDecode) (include/lzma_gpu.h).
//
// The reference reads xz strictly forward (XzUnpacker_Code, XzDec.c:604-870)
// or indexes it backwards from the footer (Xzs_ReadBackward, XzIn.c:141-306).
// Here the backward index is the plan: every block of every stream becomes
// one LZMA2 item of a single GPU batch (LzmaGpu_PlanBatchEx /
// LzmaGpu_DecodeBatchEx), followed by the filter kernels for blocks that
// carry a filter chain and the CRC-32 / CRC-64 / SHA-256 kernels for the block
// checks (the range primitives, range_capi.hip, through host_batch.h).
// The host keeps what the reference keeps outside its coders: container
// parsing with its small CRC-32s (stream header, block headers, index,
// footer) and the comparison of the computed checks with the stored fields.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_batch.h"
#include "lzma_gpu_internal.h"

static_assert(sizeof(LzmaGpuXzBlock) == 104, "LzmaGpuXzBlock layout (lzmagpu.py XzBlock)");

using namespace lzgpu_host;

namespace {

constexpr size_t kXzHeader = 12, kXzFooter = 12;

uint32_t le32(const Byte* p) {
  return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

// Xz_ReadVarInt (XzDec.c:30-44): 0 on failure
unsigned read_varint(const Byte* p, size_t max, uint64_t* v) {
  *v = 0;
  const unsigned limit = max > 9 ? 9 : unsigned(max);
  for (unsigned i = 0; i < limit;) {
    const Byte b = p[i];
    *v |= uint64_t(b & 0x7F) << (7 * i++);
    if ((b & 0x80) == 0) return (b == 0 && i != 1) ? 0 : i;
  }
  return 0;
}

// XzFlags_GetCheckSize (Xz.c:40-44)
uint32_t check_size(uint32_t t) { return t == 0 ? 0 : (4u << ((t - 1) / 3)); }

// One stream, read backwards from the footer ending at `end` (Xz_ReadBackward,
// XzIn.c:141-224); blocks appended in stream order; *start = stream start.
SRes index_stream(const Byte* f, size_t end, uint32_t stream, std::vector<LzmaGpuXzBlock>* out,
                  size_t* start) {
  if ((end & 3) != 0 || end < kXzFooter) return SZ_ERROR_NO_ARCHIVE;
  const Byte* ft = f + end - kXzFooter;
  if (ft[10] != 'Y' || ft[11] != 'Z') return SZ_ERROR_NO_ARCHIVE;
  const uint32_t flags = (uint32_t(ft[8]) << 8) | ft[9];
  if (flags > 0xF) return SZ_ERROR_UNSUPPORTED;
  if (le32(ft) != crc32_host(ft + 4, 6)) return SZ_ERROR_ARCHIVE;
  const uint64_t index_size = (uint64_t(le32(ft + 4)) + 1) << 2;
  if (index_size > end - kXzFooter) return SZ_ERROR_ARCHIVE;
  const size_t ix = end - kXzFooter - size_t(index_size);
  // Xz_ReadIndex2 (XzIn.c:62-106)
  const Byte* b = f + ix;
  size_t size = size_t(index_size);
  if (size < 5 || b[0] != 0) return SZ_ERROR_ARCHIVE;
  size -= 4;
  if (crc32_host(b, size) != le32(b + size)) return SZ_ERROR_ARCHIVE;
  size_t pos = 1;
  uint64_t nblocks;
  unsigned s = read_varint(b + pos, size - pos, &nblocks);
  if (s == 0) return SZ_ERROR_ARCHIVE;
  pos += s;
  if (nblocks * 2 > size) return SZ_ERROR_ARCHIVE;
  std::vector<uint64_t> unpadded(nblocks), unpack(nblocks);
  uint64_t packed_total = 0;
  for (uint64_t i = 0; i < nblocks; ++i) {
    s = read_varint(b + pos, size - pos, &unpadded[i]);
    if (s == 0) return SZ_ERROR_ARCHIVE;
    pos += s;
    s = read_varint(b + pos, size - pos, &unpack[i]);
    if (s == 0) return SZ_ERROR_ARCHIVE;
    pos += s;
    if (unpadded[i] == 0) return SZ_ERROR_ARCHIVE;
    packed_total += (unpadded[i] + 3) & ~uint64_t(3);
    if (packed_total >= (uint64_t(1) << 62)) return SZ_ERROR_ARCHIVE;
  }
  while ((pos & 3) != 0)
    if (b[pos++] != 0) return SZ_ERROR_ARCHIVE;
  if (pos != size) return SZ_ERROR_ARCHIVE;
  // stream header (Xz_ReadHeader / Xz_ParseHeader, XzIn.c:10-17, XzDec.c:482-489)
  const uint64_t sum = kXzHeader + packed_total + index_size;
  if (sum > end - kXzFooter) return SZ_ERROR_ARCHIVE;
  const size_t st = end - kXzFooter - size_t(sum);
  static const Byte kSig[6] = {0xFD, '7', 'z', 'X', 'Z', 0};
  if (memcmp(f + st, kSig, 6) != 0) return SZ_ERROR_NO_ARCHIVE;
  if (crc32_host(f + st + 6, 2) != le32(f + st + 8)) return SZ_ERROR_NO_ARCHIVE;
  const uint32_t hflags = (uint32_t(f[st + 6]) << 8) | f[st + 7];
  if (hflags > 0xF) return SZ_ERROR_UNSUPPORTED;
  if (hflags != flags) return SZ_ERROR_ARCHIVE;
  const uint32_t ctype = flags & 0xF, csize = check_size(ctype);
  // blocks (XzBlock_Parse, XzDec.c:505-556)
  size_t at = st + kXzHeader;
  for (uint64_t i = 0; i < nblocks; ++i) {
    const Byte* h = f + at;
    const uint32_t hsize = (uint32_t(h[0]) << 2) + 4;
    if (h[0] == 0 || uint64_t(hsize) + csize >= unpadded[i]) return SZ_ERROR_ARCHIVE;
    const uint32_t hs = hsize - 4;
    if (crc32_host(h, hs) != le32(h + hs)) return SZ_ERROR_ARCHIVE;
    size_t p = 1;
    const Byte bflags = h[p++];
    uint64_t v;
    const uint64_t pack = unpadded[i] - hsize - csize;
    if (bflags & 0x40) {
      s = read_varint(h + p, hs - p, &v);
      if (s == 0 || v == 0 || v != pack) return SZ_ERROR_ARCHIVE;
      p += s;
    }
    if (bflags & 0x80) {
      s = read_varint(h + p, hs - p, &v);
      if (s == 0 || v != unpack[i]) return SZ_ERROR_ARCHIVE;
      p += s;
    }
    const int nf = (bflags & 3) + 1;
    uint64_t ids[4];
    uint32_t psz[4];
    const Byte* props[4];
    for (int k = 0; k < nf; ++k) {
      s = read_varint(h + p, hs - p, &ids[k]);
      if (s == 0) return SZ_ERROR_ARCHIVE;
      p += s;
      s = read_varint(h + p, hs - p, &v);
      if (s == 0) return SZ_ERROR_ARCHIVE;
      p += s;
      if (v > hs - p || v > 20) return SZ_ERROR_ARCHIVE;
      psz[k] = uint32_t(v);
      props[k] = h + p;
      p += size_t(v);
    }
    while (p < hs)
      if (h[p++] != 0) return SZ_ERROR_ARCHIVE;
    LzmaGpuXzBlock blk;
    memset(&blk, 0, sizeof blk);
    // chains: up to three of Delta / x86 / PPC / IA64 / ARM / ARMT / SPARC, then
    // LZMA2 (XZ_ID_LZMA2 0x21); props validated as BraState_SetProps does
    // (XzDec.c:71-109)
    const int last = nf - 1;
    if (ids[last] != 0x21 || psz[last] != 1 || props[last][0] > 40) return SZ_ERROR_UNSUPPORTED;
    blk.num_filters = uint32_t(last);
    for (int k = 0; k < last; ++k) {
      const uint64_t id = ids[k];
      uint32_t prop = 0;
      if (id == 3) {  // XZ_ID_Delta: one byte, distance = byte + 1
        if (psz[k] != 1) return SZ_ERROR_UNSUPPORTED;
        prop = uint32_t(props[k][0]) + 1;
      } else if (id >= 4 && id <= 9) {
        if (psz[k] == 4) {
          prop = le32(props[k]);
          const uint32_t align = id == 6 ? 0xF : (id == 8 ? 1 : (id == 4 ? 0 : 3));
          if (prop & align) return SZ_ERROR_UNSUPPORTED;
        } else if (psz[k] != 0) {
          return SZ_ERROR_UNSUPPORTED;
        }
        if (id == 4) {
          blk.x86 = 1;
          blk.x86_ip = prop;
        }
      } else {
        return SZ_ERROR_UNSUPPORTED;
      }
      blk.filter_id[k] = uint32_t(id);
      blk.filter_prop[k] = prop;
    }
    blk.header_off = at;
    blk.data_off = at + hsize;
    blk.pack_size = pack;
    blk.unpack_size = unpack[i];
    blk.check_off = at + ((uint64_t(hsize) + pack + 3) & ~uint64_t(3));
    blk.check_type = ctype;
    blk.check_size = csize;
    blk.lzma2_prop = props[last][0];
    blk.stream = stream;
    out->push_back(blk);
    at += size_t((unpadded[i] + 3) & ~uint64_t(3));
  }
  *start = st;
  return SZ_OK;
}

SRes index_file(const Byte* f, size_t size, std::vector<LzmaGpuXzBlock>* blocks,
                uint64_t* total) {
  std::vector<std::vector<LzmaGpuXzBlock>> streams;
  size_t end = size;
  if (size < kXzFooter + kXzHeader) return SZ_ERROR_NO_ARCHIVE;
  for (;;) {
    // stream padding: zero bytes in multiples of 4 (XzIn.c:153-187)
    size_t e = end;
    while (e > 0 && f[e - 1] == 0) --e;
    if (e != end) {
      if (((end - e) & 3) != 0) return SZ_ERROR_NO_ARCHIVE;
      end = e;
    }
    std::vector<LzmaGpuXzBlock> one;
    size_t start = 0;
    const SRes r = index_stream(f, end, 0, &one, &start);
    if (r != SZ_OK) return r;
    streams.push_back(std::move(one));
    if (start == 0) break;
    end = start;
  }
  blocks->clear();
  uint64_t dst = 0;
  for (size_t k = streams.size(); k-- > 0;) {
    for (LzmaGpuXzBlock& b : streams[k]) {
      b.stream = uint32_t(streams.size() - 1 - k);
      b.dst_off = dst;
      // The reference guards this sum (ADD_SIZE_CHECH in Xzs_GetUnpackSize,
      // XzIn.c:43-44, 254-261) and leaves its caller to look at the result.
      // Here the sum becomes device ranges, so a total that wraps or reaches
      // 2^63 ends the index, with the code XzIn.c:208-211 gives its own
      // oversized sums.  Every caller of the index is behind this line.
      if (b.unpack_size >= (uint64_t(1) << 63) - dst) return SZ_ERROR_ARCHIVE;
      dst += b.unpack_size;
      blocks->push_back(b);
    }
  }
  *total = dst;
  return SZ_OK;
}

}  // namespace

static SRes xz_index(const Byte* file, size_t size, LzmaGpuXzBlock* blocks, size_t cap,
                     size_t* n_blocks, uint64_t* unpack_total) {
  std::vector<LzmaGpuXzBlock> v;
  uint64_t total = 0;
  const SRes r = index_file(file, size, &v, &total);
  if (n_blocks) *n_blocks = r == SZ_OK ? v.size() : 0;
  if (unpack_total) *unpack_total = r == SZ_OK ? total : 0;
  if (r != SZ_OK) return r;
  if (blocks)
    for (size_t i = 0; i < v.size() && i < cap; ++i) blocks[i] = v[i];
  return SZ_OK;
}

static SRes xz_decode(Byte* dest, SizeT* destLen, const Byte* file, size_t size,
                      int64_t* bad_block) {
  const SizeT cap = *destLen;
  *destLen = 0;
  if (bad_block) *bad_block = -1;
  std::vector<LzmaGpuXzBlock> blk;
  uint64_t total = 0;
  SRes r = index_file(file, size, &blk, &total);
  if (r != SZ_OK) return r;
  if (total > cap) return SZ_ERROR_OUTPUT_EOF;
  const size_t n = blk.size();
  if (n == 0) return SZ_OK;
  if (!ensure_device()) return SZ_ERROR_FAIL;
  // per-block failure in the reference's order: data, then padding, then check
  std::vector<int> fail(n, SZ_OK);
  for (size_t i = 0; i < n; ++i) {
    for (uint64_t p = blk[i].data_off + blk[i].pack_size; p < blk[i].check_off; ++p)
      if (file[p] != 0) fail[i] = SZ_ERROR_CRC;
  }
  // one LZMA2 item per block, FINISH_END at exactly its indexed size
  std::vector<LzmaGpuStreamDesc> descs(n);
  for (size_t i = 0; i < n; ++i) {
    LzmaGpuStreamDesc& d = descs[i];
    memset(&d, 0, sizeof d);
    d.src_off = blk[i].data_off;
    d.src_len = blk[i].pack_size;
    d.dst_off = blk[i].dst_off;
    d.dst_cap = blk[i].unpack_size;
    d.props[0] = Byte(blk[i].lzma2_prop);
    d.props_size = 1;
    d.finish_mode = LZMA_FINISH_END;
    d.kind = LZMA_GPU_KIND_LZMA2;
  }
  std::vector<uint32_t> order(n);
  LzmaGpuPlan plan;
  if ((r = LzmaGpu_PlanBatchEx(descs.data(), n, order.data(), &plan)) != SZ_OK) return r;
  // check ranges (after the filters): the CRC-32, the CRC-64 and the SHA-256 blocks
  struct Kind {
    unsigned type, bytes;
    std::vector<size_t> idx;
    std::vector<uint64_t> off, len;
    RangeChecks checks;
  } kinds[3] = {{LZMA_GPU_XZ_CHECK_CRC32, 4, {}, {}, {}, {}},
                {LZMA_GPU_XZ_CHECK_CRC64, 8, {}, {}, {}, {}},
                {LZMA_GPU_XZ_CHECK_SHA256, 32, {}, {}, {}, {}}};
  for (size_t i = 0; i < n; ++i)
    for (Kind& k : kinds)
      if (blk[i].check_type == k.type) {
        k.idx.push_back(i);
        k.off.push_back(blk[i].dst_off);
        k.len.push_back(blk[i].unpack_size);
      }
  DevArr<Byte> d_src, d_dst, d_ws;
  DevArr<LzmaGpuStreamDesc> d_desc;
  DevArr<uint32_t> d_order;
  DevArr<LzmaGpuResult> d_res;
  if ((r = alloc_all("XzDecode", d_src, size, d_dst, size_t(total), d_ws,
                     size_t(plan.workspace_bytes), d_res, n)) != SZ_OK)
    return r;
  if (!hip_ok(hipMemcpy(d_src.p, file, size, hipMemcpyHostToDevice), "XzDecode H2D"))
    return SZ_ERROR_FAIL;
  if ((r = upload(d_desc, descs, "XzDecode")) != SZ_OK ||
      (r = upload(d_order, order, "XzDecode")) != SZ_OK)
    return r;
  for (Kind& k : kinds)
    if ((r = k.checks.prepare("XzDecode", k.bytes, k.off, k.len)) != SZ_OK) return r;
  if ((r = LzmaGpu_DecodeBatchEx(&plan, d_desc.p, d_order.p, d_src.p, d_dst.p, d_ws.p, d_res.p,
                                 nullptr)) != SZ_OK)
    return r;
  // filter chains, last filter first (MixCoder order, XzDec.c:574-585): at each
  // depth, one batch per filter kind over the blocks that have that many
  for (uint32_t depth = 0; depth < 3; ++depth) {
    for (uint32_t kind = 3; kind <= 9; ++kind) {
      std::vector<uint64_t> fo, fl;
      std::vector<uint32_t> fp;  // start ip / delta distance
      for (size_t i = 0; i < n; ++i) {
        const uint32_t nf = blk[i].num_filters;
        if (nf > depth && blk[i].filter_id[nf - 1 - depth] == kind) {
          fo.push_back(blk[i].dst_off);
          fl.push_back(blk[i].unpack_size);
          fp.push_back(blk[i].filter_prop[nf - 1 - depth]);
        }
      }
      if (fo.empty()) continue;
      FilterJob job;
      if ((r = queue_filter("XzDecode", job, kind, d_dst.p, fo, fl, fp.data(), 0)) != SZ_OK)
        return r;
      if (!hip_ok(hipDeviceSynchronize(), "XzDecode filters")) return SZ_ERROR_FAIL;
    }
  }
  for (Kind& k : kinds)
    if ((r = k.checks.launch(d_dst.p)) != SZ_OK) return r;
  std::vector<LzmaGpuResult> res(n);
  std::vector<Byte> value[3];
  if (!hip_ok(hipDeviceSynchronize(), "XzDecode kernels") || !download(res, d_res.p, "XzDecode D2H"))
    return SZ_ERROR_FAIL;
  for (size_t t = 0; t < 3; ++t) {
    value[t].resize(kinds[t].idx.size() * kinds[t].bytes);
    if (!kinds[t].checks.fetch(value[t].data(), "XzDecode D2H")) return SZ_ERROR_FAIL;
  }
  if (!hip_ok(hipMemcpy(dest, d_dst.p, total, hipMemcpyDeviceToHost), "XzDecode D2H"))
    return SZ_ERROR_FAIL;
  for (size_t i = 0; i < n; ++i) {
    const LzmaGpuResult& q = res[i];
    if (q.res != SZ_OK || q.status != LZMA_STATUS_FINISHED_WITH_MARK ||
        q.dest_len != blk[i].unpack_size || q.src_len != blk[i].pack_size)
      fail[i] = SZ_ERROR_DATA;
  }
  // the values are little-endian on the device as in the file
  for (size_t t = 0; t < 3; ++t)
    for (size_t k = 0; k < kinds[t].idx.size(); ++k) {
      const size_t i = kinds[t].idx[k], nb = kinds[t].bytes;
      if (fail[i] == SZ_OK && memcmp(&value[t][nb * k], file + blk[i].check_off, nb) != 0)
        fail[i] = SZ_ERROR_CRC;
    }
  for (size_t i = 0; i < n; ++i)
    if (fail[i] != SZ_OK) {
      if (bad_block) *bad_block = int64_t(i);
      return fail[i];
    }
  *destLen = SizeT(total);
  return SZ_OK;
}

// C ABI: no exception crosses it (host allocation failure -> SZ_ERROR_MEM).
SRes LzmaGpu_XzIndex(const Byte* file, size_t size, LzmaGpuXzBlock* blocks, size_t cap,
                     size_t* n_blocks, uint64_t* unpack_total) {
  return guarded("xz: host allocation failed",
                 [&]() { return xz_index(file, size, blocks, cap, n_blocks, unpack_total); });
}

SRes LzmaGpu_XzDecode(Byte* dest, SizeT* destLen, const Byte* file, size_t size,
                      int64_t* bad_block) {
  return guarded("xz: host allocation failed",
                 [&]() { return xz_decode(dest, destLen, file, size, bad_block); });
}
