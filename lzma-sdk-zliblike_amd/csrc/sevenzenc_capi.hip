// sevenzenc_capi.hip -- C ABI of the 7z writer (include/lzma_gpu.h): the plan
// (items -> folders and pieces), the header writer, the pack stage's device
// entry, and LzmaGpu_7zWrite, which runs the CRC, filter, encode and pack
// batches over every folder of the archive and writes the archive.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <numeric>
#include <string.h>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "bcj2enc_device.h"
#include "bcj2enc_internal.h"
#include "host_batch.h"
#include "lzma2enc_internal.h"
#include "lzma_gpu_internal.h"
#include "lzmaenc_internal.h"
#include "ppmd7_internal.h"
#include "sevenz_pack_device.h"
#include "sevenzenc_internal.h"

using namespace lzgpu_host;

static_assert(sizeof(LzmaGpu7zItem) == 32 && sizeof(LzmaGpu7zMethod) == 88 &&
                  sizeof(LzmaGpu7zWriteOptions) == 16 && sizeof(LzmaGpu7zWriteStats) == 112 &&
                  sizeof(SzGpuPackPiece) == 32 && sizeof(SzGpuPackArgs) == 152 &&
                  sizeof(LzmaGpu7zBcj2Info) == 72,
              "7z writer ABI");

namespace {

constexpr uint64_t kCopy = 0, kLzma = 0x030101, kLzma2 = 0x21, kPpmd = 0x030401;
constexpr uint64_t kBcjX86 = 0x03030103, kBcjArm = 0x03030501;
constexpr uint64_t kBcj2 = 0x0303011B;
constexpr uint32_t kFilterX86 = 4, kFilterArm = 7, kFilterBcj2 = LZMA_GPU_7Z_FILTER_BCJ2;
// 7z.h:17-45
constexpr uint8_t kEnd = 0, kHeader = 1, kMainStreamsInfo = 4, kFilesInfo = 5, kPackInfo = 6,
                  kUnpackInfo = 7, kSubStreamsInfo = 8, kSize = 9, kCrc = 10, kFolder = 11,
                  kCodersUnpackSize = 12, kNumUnpackStream = 13, kEmptyStream = 14,
                  kEmptyFile = 15, kName = 17, kEncodedHeader = 23;
// LZMA and PPMd7 streams encoded again after SZ_ERROR_OUTPUT_EOF: at most this
// many more batches per kind, then the call fails
constexpr unsigned kReencodeRounds = 2;

// The first slot holds what compresses at all.  The reference's fast mode
// turns random bytes into len * 1.0145 + 5 (measured, 256 bytes to 64 KiB), so
// incompressible streams above about 9 KiB take the second round: they pay a
// second encode, and everything else a slot of 1.008 len instead of 1.33 len.
uint64_t first_slot(uint64_t len) { return len + (len >> 7) + 64; }
uint64_t lzma_retry_slot(uint64_t len, unsigned round) {
  return round == 1 ? len + len / 3 + 128 : 2 * len + 1024;
}

bool has_data(const LzmaGpu7zItem& it) {
  return it.size != 0 && !(it.flags & LZMA_GPU_7Z_ITEM_DIR);
}

struct Method {
  uint64_t id = 0;
  uint32_t filter = 0;
  LzmaEncGpuStreamDesc proto;  // LZMA, LZMA2
  uint64_t block_size = 0;     // LZMA2
  uint32_t order = 0, mem = 0;  // PPMd7
  uint8_t props[5] = {0, 0, 0, 0, 0};
  uint32_t props_size = 0;
  LzmaEncGpuStreamDesc target_proto;  // BCJ2: the CALL and JMP coders
  uint8_t target_props[5] = {0, 0, 0, 0, 0};
};

struct FolderPlan {
  uint32_t method = 0;  // index
  uint32_t first_item = 0, num_files = 0;
  uint64_t off = 0, size = 0;
};

struct Plan {
  std::vector<Method> methods;
  std::vector<FolderPlan> folders;
  uint64_t n_data = 0, n_pieces = 0, pack_bound = 0, n_bcj2 = 0;
};

SRes resolve_method(const LzmaGpu7zMethod& in, Method& m) {
  memset(&m.proto, 0, sizeof(m.proto));
  m.id = in.method;
  m.filter = in.filter;
  if (in.filter != 0 && in.filter != kFilterX86 && in.filter != kFilterArm &&
      in.filter != kFilterBcj2)
    return SZ_ERROR_PARAM;
  if (in.filter == kFilterBcj2 && (in.method == kCopy || in.method == kLzma2 || in.method == kPpmd)) {
    set_error("7z write: the BCJ2 filter is written over LZMA rows only");
    return SZ_ERROR_UNSUPPORTED;
  }
  if (in.method == kCopy) return SZ_OK;
  if (in.method == kLzma) {
    m.props_size = 5;
    const SRes r = LzmaEncGpu_DescFromProps(&in.props.lzmaProps, 0, &m.proto, m.props);
    if (r != SZ_OK || in.filter != kFilterBcj2) return r;
    // the CALL and JMP coders: lc 0, lp 2, pb 2, a dictionary of at most 1 MiB
    CLzmaEncProps t = in.props.lzmaProps;
    LzmaEncProps_Normalize(&t);
    t.lc = 0;
    t.lp = 2;
    t.pb = 2;
    if (t.dictSize > (1u << 20)) t.dictSize = 1u << 20;
    memset(&m.target_proto, 0, sizeof(m.target_proto));
    return LzmaEncGpu_DescFromProps(&t, 0, &m.target_proto, m.target_props);
  }
  if (in.method == kLzma2) {
    m.props_size = 1;
    const SRes r = Lzma2EncGpu_DescFromProps(&in.props, &m.proto, m.props);
    if (r != SZ_OK) return r;
    CLzma2EncProps norm = in.props;
    Lzma2EncProps_Normalize(&norm);
    m.block_size = norm.blockSize;
    return m.block_size ? SZ_OK : SZ_ERROR_PARAM;
  }
  if (in.method == kPpmd) {
    if (in.ppmd_order < 2 || in.ppmd_order > 64 || in.ppmd_mem_size < (1u << 11) ||
        in.ppmd_mem_size > 0xFFFFFFFFu - 36u)
      return SZ_ERROR_PARAM;
    m.order = in.ppmd_order;
    m.mem = in.ppmd_mem_size;
    m.props_size = 5;
    m.props[0] = uint8_t(m.order);
    for (int i = 0; i < 4; ++i) m.props[1 + i] = uint8_t(m.mem >> (8 * i));
    return SZ_OK;
  }
  return SZ_ERROR_PARAM;
}

uint64_t lzma2_block(const Method& m, uint64_t size) {
  return m.block_size > size ? size : m.block_size;
}

SRes make_plan(const LzmaGpu7zItem* items, size_t n, size_t src_size, size_t names_len,
               const LzmaGpu7zMethod* methods, size_t n_methods, Plan& p) {
  p.methods.resize(n_methods);
  for (size_t k = 0; k < n_methods; ++k) {
    const SRes r = resolve_method(methods[k], p.methods[k]);
    if (r != SZ_OK) return r;
  }
  if (n > 0xFFFFFFFEull) return SZ_ERROR_PARAM;
  bool have_prev = false;
  for (size_t i = 0; i < n; ++i) {
    const LzmaGpu7zItem& it = items[i];
    if (it.flags & ~uint32_t(LZMA_GPU_7Z_ITEM_DIR | LZMA_GPU_7Z_ITEM_JOIN)) return SZ_ERROR_PARAM;
    if ((it.flags & LZMA_GPU_7Z_ITEM_DIR) && it.size != 0) return SZ_ERROR_PARAM;
    if (it.name_len == 0 || it.name_off > names_len || it.name_len > names_len - it.name_off)
      return SZ_ERROR_PARAM;
    if (!has_data(it)) continue;
    if (it.method >= n_methods || it.src_off > src_size || it.size > src_size - it.src_off)
      return SZ_ERROR_PARAM;
    ++p.n_data;
    if (it.flags & LZMA_GPU_7Z_ITEM_JOIN) {
      if (!have_prev) return SZ_ERROR_PARAM;
      FolderPlan& f = p.folders.back();
      if (it.method != f.method || it.src_off != f.off + f.size) return SZ_ERROR_PARAM;
      f.size += it.size;
      ++f.num_files;
    } else {
      FolderPlan f;
      f.method = it.method;
      f.first_item = uint32_t(i);
      f.num_files = 1;
      f.off = it.src_off;
      f.size = it.size;
      p.folders.push_back(f);
      have_prev = true;
    }
  }
  for (const FolderPlan& f : p.folders) {
    const Method& m = p.methods[f.method];
    if (m.id == kCopy) {
      p.n_pieces += 1;
      p.pack_bound += f.size;
    } else if (m.id == kLzma2) {
      const uint64_t b = lzma2_block(m, f.size);
      if (b >= (uint64_t(1) << 31)) {
        set_error("7z write: an LZMA2 block of 2^31 bytes or more is not supported");
        return SZ_ERROR_UNSUPPORTED;
      }
      const uint64_t blocks = (f.size + b - 1) / b;
      p.n_pieces += blocks;
      p.pack_bound += f.size + blocks * (Lzma2EncGpu_BlockBound(size_t(b)) - b) + 1;
    } else {
      if (f.size >= (uint64_t(1) << 31)) {
        set_error("7z write: an LZMA or PPMd7 folder of 2^31 bytes or more is not supported");
        return SZ_ERROR_UNSUPPORTED;
      }
      if (m.filter == kFilterBcj2) {  // main, rc, call, jump
        uint64_t b[4];
        Bcj2EncGpu_Bound(f.size, b);
        ++p.n_bcj2;
        p.n_pieces += 4;
        p.pack_bound += lzma_retry_slot(b[0], kReencodeRounds) + b[3] +
                        lzma_retry_slot(b[1], kReencodeRounds) +
                        lzma_retry_slot(b[2], kReencodeRounds);
        continue;
      }
      p.n_pieces += 1;
      p.pack_bound += lzma_retry_slot(f.size, kReencodeRounds);
    }
  }
  if (p.n_pieces > 0x7FFFFFFFull) {
    set_error("7z write: 2^31 pieces or more");
    return SZ_ERROR_UNSUPPORTED;
  }
  return SZ_OK;
}

void fill_folder(const Plan& p, size_t k, LzmaGpu7zFolder& o) {
  const FolderPlan& f = p.folders[k];
  const Method& m = p.methods[f.method];
  memset(&o, 0, sizeof(o));
  o.unpack_size = f.size;
  o.dst_off = f.off;
  o.method = m.id;
  o.x86 = m.filter == kFilterX86 ? 1 : 0;
  o.first_file = f.first_item;
  o.num_files = f.num_files;
  o.num_coders = m.filter == kFilterBcj2 ? 4 : (m.filter ? 2 : 1);
  o.props_size = m.props_size;
  memcpy(o.props, m.props, m.props_size);
}

uint64_t header_bound(size_t n_folders, size_t n_bcj2, size_t n_items, size_t names_len) {
  return 64 + uint64_t(n_folders) * 64 + uint64_t(n_bcj2) * 128 + uint64_t(n_items) * 15 +
         uint64_t(names_len) * 2;
}

// ---------------------------------------------------------------- the header

typedef std::vector<uint8_t> Bytes;

// SzReadNumber's inverse (7zIn.c:348-369)
void put_number(Bytes& o, uint64_t v) {
  for (unsigned k = 0; k < 8; ++k) {
    if ((v >> (8 * k)) < (uint64_t(1) << (7 - k))) {
      o.push_back(uint8_t(((0xFF00u >> k) & 0xFFu) | (v >> (8 * k))));
      for (unsigned j = 0; j < k; ++j) o.push_back(uint8_t(v >> (8 * j)));
      return;
    }
  }
  o.push_back(0xFF);
  for (unsigned j = 0; j < 8; ++j) o.push_back(uint8_t(v >> (8 * j)));
}
void put32(Bytes& o, uint32_t v) {
  for (int i = 0; i < 4; ++i) o.push_back(uint8_t(v >> (8 * i)));
}
void put_bools(Bytes& o, const std::vector<bool>& v) {
  const size_t at = o.size();
  o.resize(at + (v.size() + 7) / 8, 0);
  for (size_t i = 0; i < v.size(); ++i)
    if (v[i]) o[at + i / 8] |= uint8_t(0x80 >> (i % 8));
}
void put_coder(Bytes& o, uint64_t id, const uint8_t* props, uint32_t props_size) {
  unsigned idn = 1;
  while (idn < 8 && (id >> (8 * idn))) ++idn;
  o.push_back(uint8_t(idn | (props_size ? 0x20 : 0)));
  for (unsigned j = idn; j-- > 0;) o.push_back(uint8_t(id >> (8 * j)));
  if (props_size) {
    put_number(o, props_size);
    o.insert(o.end(), props, props + props_size);
  }
}

// streams_info of the layout helper: pack info, the folders' coders and unpack
// sizes, folder CRCs where defined; `sub`: SubStreamsInfo with the sizes and
// CRCs of `files` (size, crc per data file, in folder order)
struct DataFile {
  uint64_t size;
  uint32_t crc;
};
void put_streams_info(Bytes& o, const LzmaGpu7zFolder* folders, size_t nf, uint64_t pack_pos,
                      const std::vector<DataFile>* files, const LzmaGpu7zBcj2Info* bcj2 = nullptr) {
  size_t n_four = 0;
  for (size_t k = 0; k < nf; ++k) n_four += folders[k].num_coders == 4;
  o.push_back(kPackInfo);
  put_number(o, pack_pos);
  put_number(o, nf + 3 * n_four);
  o.push_back(kSize);
  for (size_t k = 0, b = 0; k < nf; ++k) {
    if (folders[k].num_coders == 4) {
      for (int j = 0; j < 4; ++j) put_number(o, bcj2[b].pack_size[j]);
      ++b;
    } else {
      put_number(o, folders[k].pack_size);
    }
  }
  o.push_back(kEnd);
  o.push_back(kUnpackInfo);
  o.push_back(kFolder);
  put_number(o, nf);
  o.push_back(0);  // external
  for (size_t k = 0, b = 0; k < nf; ++k) {
    const LzmaGpu7zFolder& f = folders[k];
    if (f.num_coders == 4) {
      // coders 0, 1, 2 = jump, call, main; coder 3 = BCJ2 with 4 in, 1 out; bind
      // pairs in <- out; the pack streams' in indices (7zDec.c:303-319)
      const LzmaGpu7zBcj2Info& i = bcj2[b++];
      put_number(o, 4);
      put_coder(o, kLzma, i.jump_props, 5);
      put_coder(o, kLzma, i.call_props, 5);
      put_coder(o, f.method, f.props, f.props_size);
      o.push_back(uint8_t(4 | 0x10));
      for (unsigned j = 4; j-- > 0;) o.push_back(uint8_t(kBcj2 >> (8 * j)));
      put_number(o, 4);
      put_number(o, 1);
      static const uint8_t kBind[6] = {5, 0, 4, 1, 3, 2}, kPack[4] = {2, 6, 1, 0};
      for (uint8_t v : kBind) put_number(o, v);
      for (uint8_t v : kPack) put_number(o, v);
      continue;
    }
    put_number(o, f.num_coders == 2 ? 2 : 1);
    put_coder(o, f.method, f.props, f.props_size);
    if (f.num_coders == 2) {  // coder 1 = the filter; bind pair: in 1 <- out 0
      put_coder(o, f.x86 ? kBcjX86 : kBcjArm, nullptr, 0);
      put_number(o, 1);
      put_number(o, 0);
    }
  }
  o.push_back(kCodersUnpackSize);
  bool any_crc = false;
  for (size_t k = 0, b = 0; k < nf; ++k) {
    if (folders[k].num_coders == 4) {
      for (int j = 0; j < 3; ++j) put_number(o, bcj2[b].unpack_size[j]);
      ++b;
    }
    put_number(o, folders[k].unpack_size);
    if (folders[k].num_coders == 2) put_number(o, folders[k].unpack_size);
    any_crc = any_crc || folders[k].crc_defined;
  }
  if (any_crc) {
    o.push_back(kCrc);
    o.push_back(0);
    std::vector<bool> v(nf);
    for (size_t k = 0; k < nf; ++k) v[k] = folders[k].crc_defined != 0;
    put_bools(o, v);
    for (size_t k = 0; k < nf; ++k)
      if (folders[k].crc_defined) put32(o, folders[k].crc);
  }
  o.push_back(kEnd);
  if (files) {
    o.push_back(kSubStreamsInfo);
    o.push_back(kNumUnpackStream);  // always written
    for (size_t k = 0; k < nf; ++k) put_number(o, folders[k].num_files);
    o.push_back(kSize);
    size_t at = 0;
    for (size_t k = 0; k < nf; ++k) {
      for (uint32_t j = 0; j + 1 < folders[k].num_files; ++j) put_number(o, (*files)[at + j].size);
      at += folders[k].num_files;
    }
    o.push_back(kCrc);
    o.push_back(1);
    at = 0;
    for (size_t k = 0; k < nf; ++k) {
      const bool known = folders[k].num_files == 1 && folders[k].crc_defined;
      for (uint32_t j = 0; j < folders[k].num_files && !known; ++j) put32(o, (*files)[at + j].crc);
      at += folders[k].num_files;
    }
    o.push_back(kEnd);
  }
  o.push_back(kEnd);
}

bool folder_ok(const LzmaGpu7zFolder& f) {
  return (f.num_coders == 1 || f.num_coders == 2) && f.props_size <= sizeof(f.props);
}

SRes build_header(const LzmaGpu7zFolder* folders, size_t nf, const LzmaGpu7zItem* items, size_t n,
                  const uint32_t* file_crcs, const UInt16* names, size_t names_len, Bytes& o,
                  const LzmaGpu7zBcj2Info* bcj2 = nullptr, size_t n_bcj2 = 0) {
  std::vector<DataFile> files;
  size_t n_empty = 0;
  for (size_t i = 0; i < n; ++i) {
    const LzmaGpu7zItem& it = items[i];
    if (it.name_len == 0 || it.name_off > names_len || it.name_len > names_len - it.name_off ||
        names[it.name_off + it.name_len - 1] != 0)
      return SZ_ERROR_PARAM;
    if (has_data(it))
      files.push_back(DataFile{it.size, file_crcs ? file_crcs[i] : 0});
    else
      ++n_empty;
  }
  // the folders' files are the data items in order, their sizes the unpack size
  size_t at = 0, n_four = 0;
  for (size_t k = 0; k < nf; ++k) {
    if (folders[k].num_coders == 4) {  // only with its entry, and LZMA as the main coder
      if (n_four >= n_bcj2 || folders[k].method != kLzma || folders[k].props_size != 5)
        return SZ_ERROR_PARAM;
      ++n_four;
    } else if (!folder_ok(folders[k])) {
      return SZ_ERROR_PARAM;
    }
    if (folders[k].num_files > files.size() - at) return SZ_ERROR_PARAM;
    uint64_t sum = 0;
    for (uint32_t j = 0; j < folders[k].num_files; ++j) sum += files[at + j].size;
    if (sum != folders[k].unpack_size) return SZ_ERROR_PARAM;
    at += folders[k].num_files;
  }
  if (at != files.size()) return SZ_ERROR_PARAM;
  o.push_back(kHeader);
  o.push_back(kMainStreamsInfo);
  put_streams_info(o, folders, nf, 0, &files, bcj2);
  o.push_back(kFilesInfo);
  put_number(o, n);
  if (n_empty) {
    std::vector<bool> v(n), e;
    for (size_t i = 0; i < n; ++i) {
      v[i] = !has_data(items[i]);
      if (v[i]) e.push_back(!(items[i].flags & LZMA_GPU_7Z_ITEM_DIR));
    }
    o.push_back(kEmptyStream);
    put_number(o, (v.size() + 7) / 8);
    put_bools(o, v);
    o.push_back(kEmptyFile);
    put_number(o, (e.size() + 7) / 8);
    put_bools(o, e);
  }
  uint64_t units = 0;
  for (size_t i = 0; i < n; ++i) units += items[i].name_len;
  o.push_back(kName);
  put_number(o, units * 2 + 1);
  o.push_back(0);  // external
  for (size_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < items[i].name_len; ++j) {
      const UInt16 c = names[items[i].name_off + j];
      o.push_back(uint8_t(c));
      o.push_back(uint8_t(c >> 8));
    }
  o.push_back(kEnd);
  o.push_back(kEnd);
  return SZ_OK;
}

SRes build_stub(const LzmaGpu7zFolder* folders, size_t nf, Bytes& o) {
  if (nf != 1 || !folder_ok(folders[0])) return SZ_ERROR_PARAM;
  o.push_back(kEncodedHeader);
  put_streams_info(o, folders, 1, folders[0].pack_off, nullptr);
  return SZ_OK;
}

void write_sig(Byte* sig32, const Bytes& hdr, uint64_t pack_area_size) {
  static const Byte magic[8] = {'7', 'z', 0xBC, 0xAF, 0x27, 0x1C, 0, 4};
  memcpy(sig32, magic, 8);
  Byte* s = sig32 + 12;
  for (int i = 0; i < 8; ++i) s[i] = Byte(pack_area_size >> (8 * i));
  for (int i = 0; i < 8; ++i) s[8 + i] = Byte(uint64_t(hdr.size()) >> (8 * i));
  const uint32_t hc = crc32_host(hdr.data(), hdr.size());
  for (int i = 0; i < 4; ++i) s[16 + i] = Byte(hc >> (8 * i));
  const uint32_t sc = crc32_host(s, 20);
  for (int i = 0; i < 4; ++i) sig32[8 + i] = Byte(sc >> (8 * i));
}

// ---------------------------------------------------------------- the device pipeline

// The streams of one kind of one round in launch order (longest first), with
// workspace offsets that restart at every cut of the plan.
template <class Desc>
struct KindBatch {
  std::vector<Desc> d;
  std::vector<uint32_t> piece;  // d[k]'s piece
  LaunchPlan plan;
};

template <class Desc, class Slice>
SRes lay_out(KindBatch<Desc>& b, uint64_t limit, Slice slice) {
  if (!launch_plan(b.d.size(), [&](uint32_t i) { return b.d[i].src_len; },
                   [&](uint32_t i) { return slice(b.d[i]); }, limit, b.plan)) {
    set_error("7z write: one stream's workspace slice exceeds the limit");
    return SZ_ERROR_MEM;
  }
  b.d = in_launch_order(b.d.data(), b.plan);
  std::vector<uint32_t> piece(b.piece.size());
  for (size_t k = 0; k < piece.size(); ++k) piece[k] = b.piece[b.plan.order[k]];
  b.piece.swap(piece);
  return SZ_OK;
}

uint64_t ppmd_slice(const Ppmd7GpuEncDesc& d) { return ppmd7_slice_bytes(d.mem_size); }

struct Device {
  DevArr<uint8_t> src, slots, ws, out;
  DevArr<uint8_t> retry[kReencodeRounds];
  DevArr<LzmaEncGpuResult> lz_res, l2_res;
  DevArr<Ppmd7GpuEncResult> pp_res;
  uint64_t ws_bytes = 0;
};

// uploads one kind's descriptors and queues its launches; results land at
// res + k for d[k]
template <class Desc, class Launch>
SRes launch_kind(const char* what, const KindBatch<Desc>& b, DevArr<Desc>& g, uint64_t* launches,
                 Launch launch) {
  if (b.d.empty()) return SZ_OK;
  const SRes r = upload(g, b.d, "7z write");
  if (r != SZ_OK) return r;
  return queue_launches(what, b.plan, [&](uint32_t lo, uint32_t cnt) {
    ++*launches;
    return launch(lo, cnt);
  });
}
SRes launch_lzma(const KindBatch<LzmaEncGpuStreamDesc>& b, DevArr<LzmaEncGpuStreamDesc>& g,
                 const uint8_t* src, uint8_t* dst, uint8_t* ws, LzmaEncGpuResult* res,
                 uint64_t* launches) {
  return launch_kind("7z write: LZMA encode", b, g, launches, [&](uint32_t lo, uint32_t cnt) {
    return lzmaencgpu_launch(g.p + lo, nullptr, cnt, src, dst, ws, res + lo,
                             LZMA_ENC_GPU_LANES_DEFAULT, nullptr,
                             lzmaenc_kernels(b.d.data() + lo, cnt, lzmaenc_check));
  });
}
SRes launch_lzma2(const KindBatch<LzmaEncGpuStreamDesc>& b, DevArr<LzmaEncGpuStreamDesc>& g,
                  const uint8_t* src, uint8_t* dst, uint8_t* ws, LzmaEncGpuResult* res,
                  uint64_t* launches) {
  return launch_kind("7z write: LZMA2 encode", b, g, launches, [&](uint32_t lo, uint32_t cnt) {
    return lzma2encgpu_launch(g.p, nullptr, lo, cnt, uint32_t(b.d.size()), src, dst, ws, res,
                              LZMA_ENC_GPU_LANES_DEFAULT, nullptr,
                              lzmaenc_kernels(b.d.data() + lo, cnt, lzma2enc_check));
  });
}
SRes launch_ppmd(const KindBatch<Ppmd7GpuEncDesc>& b, DevArr<Ppmd7GpuEncDesc>& g,
                 const uint8_t* src, uint8_t* dst, uint8_t* ws, Ppmd7GpuEncResult* res,
                 uint64_t* launches) {
  return launch_kind("7z write: PPMd7 encode", b, g, launches, [&](uint32_t lo, uint32_t cnt) {
    return ppmd7encgpu_launch(g.p + lo, cnt, src, dst, ws, res + lo, nullptr);
  });
}

// CrcCalc of every data item over the uploaded source (queued, not awaited)
SRes queue_crcs(const LzmaGpu7zItem* items, size_t n, const uint8_t* d_src, RangeChecks& j) {
  std::vector<uint64_t> off, len;
  for (size_t i = 0; i < n; ++i)
    if (has_data(items[i])) {
      off.push_back(items[i].src_off);
      len.push_back(items[i].size);
    }
  const SRes r = j.prepare("7z write", 4, off, len);
  return r == SZ_OK ? j.launch(d_src) : r;
}

// the x86 and ARM filters, encoding, in place over the filtered folders:
// x86_Convert(data, size, 0, &state0, 1) and ARM_Convert(data, size, 0, 1) per folder
SRes queue_filters(const Plan& p, uint8_t* d_src, FilterJob& x86, FilterJob& arm) {
  std::vector<uint64_t> xo, xl, ao, al;
  for (const FolderPlan& f : p.folders) {
    const uint32_t filter = p.methods[f.method].filter;
    if (filter == kFilterX86) {
      xo.push_back(f.off);
      xl.push_back(f.size);
    } else if (filter == kFilterArm) {
      ao.push_back(f.off);
      al.push_back(f.size);
    }
  }
  const SRes r = queue_filter("7z write", x86, kFilterX86, d_src, xo, xl, nullptr, 1);
  return r == SZ_OK ? queue_filter("7z write", arm, kFilterArm, d_src, ao, al, nullptr, 1) : r;
}

// a filtered folder is converted in place: its range may not meet another's
bool filtered_ranges_overlap(const Plan& p) {
  std::vector<size_t> by(p.folders.size());
  std::iota(by.begin(), by.end(), size_t(0));
  std::sort(by.begin(), by.end(),
            [&](size_t a, size_t b) { return p.folders[a].off < p.folders[b].off; });
  // in offset order a folder meets an earlier one exactly when it starts
  // before the furthest end seen (folders are never empty)
  uint64_t end_any = 0, end_filtered = 0;
  for (size_t k = 0; k < by.size(); ++k) {
    const FolderPlan& f = p.folders[by[k]];
    const uint32_t filter = p.methods[f.method].filter;
    const bool filt = filter != 0 && filter != kFilterBcj2;  // BCJ2 splits out of place
    if (f.off < end_filtered || (filt && f.off < end_any)) return true;
    end_any = std::max(end_any, f.off + f.size);
    if (filt) end_filtered = std::max(end_filtered, f.off + f.size);
  }
  return false;
}

// A BCJ2 folder's four streams (main, call, jump, rc as Bcj2GpuEncDesc has them)
// behind the uploaded source, in the same allocation
struct Bcj2Split {
  size_t folder;
  uint64_t off[4], len[4];
};
uint64_t lay_out_bcj2(const Plan& p, uint64_t at, std::vector<Bcj2Split>& v) {
  for (size_t k = 0; k < p.folders.size(); ++k) {
    if (p.methods[p.folders[k].method].filter != kFilterBcj2) continue;
    Bcj2Split b;
    uint64_t cap[4];
    Bcj2EncGpu_Bound(p.folders[k].size, cap);
    b.folder = k;
    for (int j = 0; j < 4; ++j) {
      b.off[j] = at;
      b.len[j] = cap[j];  // the capacity until the split has run
      at += cap[j];
    }
    v.push_back(b);
  }
  return at;
}
// the split of every BCJ2 folder, in launches cut by `limit`; waits and leaves
// the true lengths in v
SRes split_bcj2(const Plan& p, std::vector<Bcj2Split>& v, uint8_t* d_src, uint64_t limit) {
  if (v.empty()) return SZ_OK;
  std::vector<Bcj2GpuEncDesc> d(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    d[i].src_off = p.folders[v[i].folder].off;
    d[i].src_len = p.folders[v[i].folder].size;
    for (int j = 0; j < 4; ++j) {
      d[i].out[j].off = v[i].off[j];
      d[i].out[j].cap = v[i].len[j];
    }
  }
  LaunchPlan lp;
  if (!launch_plan(d.size(), [&](uint32_t i) { return d[i].src_len; },
                   [&](uint32_t i) { return bcj2enc::slice_bytes(d[i].src_len); },
                   limit > bcj2enc::fixed_bytes() ? limit - bcj2enc::fixed_bytes() : 0, lp)) {
    set_error("7z write: one BCJ2 folder's scratch exceeds the limit");
    return SZ_ERROR_MEM;
  }
  const std::vector<Bcj2GpuEncDesc> ordered = in_plan_order(d.data(), lp);
  DevArr<Bcj2GpuEncDesc> g_d;
  DevArr<Bcj2GpuEncResult> g_r;
  DevArr<uint8_t> g_ws;
  SRes r = upload(g_d, ordered, "7z write");
  if (r == SZ_OK)
    r = alloc_all("7z write", g_r, d.size(), g_ws, size_t(lp.ws_max + bcj2enc::fixed_bytes()));
  if (r == SZ_OK)
    r = queue_launches("7z write: BCJ2 split", lp, [&](uint32_t lo, uint32_t cnt) {
      return bcj2encgpu_launch(g_d.p + lo, cnt, d_src, d_src, g_ws.p, g_r.p + lo, kBcj2EncAll,
                               nullptr);
    });
  if (r != SZ_OK) return r;
  std::vector<Bcj2GpuEncResult> res(d.size());
  if (!hip_ok(hipDeviceSynchronize(), "7z write: BCJ2 split") ||
      !download(res, g_r.p, "download BCJ2 lengths"))
    return SZ_ERROR_FAIL;
  for (size_t k = 0; k < res.size(); ++k) {
    if (res[k].res != SZ_OK) {  // the capacities are the bounds
      set_error("7z write: a BCJ2 split failed on the device");
      return SZ_ERROR_FAIL;
    }
    for (int j = 0; j < 4; ++j) v[lp.order[k]].len[j] = res[k].len[j];
  }
  return SZ_OK;
}

// the header as one more LZMA stream: the batch path with one stream
SRes encode_header_stream(const Bytes& hdr, Bytes& packed, uint8_t props5[5]) {
  CLzmaEncProps props;
  LzmaEncProps_Init(&props);
  props.level = 4;
  uint32_t dict = 1u << 12;
  while (dict < hdr.size() && dict < (1u << 26)) dict <<= 1;
  props.dictSize = dict;
  LzmaEncGpuStreamDesc d;
  memset(&d, 0, sizeof(d));
  const SRes pr = LzmaEncGpu_DescFromProps(&props, 0, &d, props5);
  if (pr != SZ_OK) return pr;
  if (hdr.size() >= (uint64_t(1) << 30)) return SZ_ERROR_UNSUPPORTED;
  d.src_len = hdr.size();
  d.dst_cap = lzma_retry_slot(hdr.size(), kReencodeRounds);
  packed.assign(size_t(d.dst_cap), 0);
  LzmaEncGpuResult r;
  r.res = SZ_ERROR_FAIL;
  r.dest_len = 0;
  const SRes er = LzmaEncGpu_EncodeBatchHost(&d, 1, hdr.data(), hdr.size(), packed.data(),
                                             packed.size(), &r, 0);
  if (er != SZ_OK) return er;
  if (r.res != SZ_OK) {
    set_error("7z write: the header's LZMA stream failed");
    return SZ_ERROR_FAIL;
  }
  packed.resize(size_t(r.dest_len));
  return SZ_OK;
}

SRes write_archive(Byte* dest, SizeT* destLen, const Byte* src, size_t src_size,
                   const LzmaGpu7zItem* items, size_t n, const UInt16* names, size_t names_len,
                   const LzmaGpu7zMethod* methods, size_t n_methods,
                   const LzmaGpu7zWriteOptions* options, LzmaGpu7zWriteStats* stats) {
  LzmaGpu7zWriteStats st;
  memset(&st, 0, sizeof(st));
  if (stats) *stats = st;
  const uint32_t flags = options ? options->flags : 0;
  if (flags & ~uint32_t(LZMA_GPU_7Z_WRITE_KNOWN_FLAGS)) return SZ_ERROR_PARAM;
  Plan p;
  const SRes plan_res = make_plan(items, n, src_size, names_len, methods, n_methods, p);
  if (plan_res != SZ_OK) return plan_res;
  for (size_t i = 0; i < n; ++i)
    if (names[items[i].name_off + items[i].name_len - 1] != 0) return SZ_ERROR_PARAM;
  if (filtered_ranges_overlap(p)) {
    set_error("7z write: a filtered folder's source range overlaps another folder's");
    return SZ_ERROR_PARAM;
  }
  if (!ensure_device()) return SZ_ERROR_FAIL;
  // stage times: the host clock, after a synchronisation when TIMINGS asks for one
  const bool timed = (flags & LZMA_GPU_7Z_WRITE_TIMINGS) != 0;
  const auto t_begin = std::chrono::steady_clock::now();
  auto t_last = t_begin;
  const auto mark = [&](int stage) {
    if (!timed) return;
    (void)hipDeviceSynchronize();
    const auto t = std::chrono::steady_clock::now();
    st.stage_ns[stage] += uint64_t(std::chrono::nanoseconds(t - t_last).count());
    t_last = t;
  };
  uint64_t limit = options ? options->workspace_limit : 0;
  if (!default_workspace_limit(limit)) return SZ_ERROR_FAIL;

  // upload, CRCs, filters and the BCJ2 split: queued on the null stream, in order
  Device g;
  std::vector<Bcj2Split> bcj2;
  const uint64_t src_alloc = lay_out_bcj2(p, src_size, bcj2);
  SRes r;
  if ((r = alloc_all("7z write", g.src, size_t(src_alloc))) != SZ_OK) return r;
  if (src_size && !hip_ok(hipMemcpy(g.src.p, src, src_size, hipMemcpyHostToDevice), "upload src"))
    return SZ_ERROR_FAIL;
  mark(LZMA_GPU_7Z_STAGE_UPLOAD);
  RangeChecks crc;
  FilterJob filt_x86, filt_arm;
  if ((r = queue_crcs(items, n, g.src.p, crc)) != SZ_OK) return r;
  mark(LZMA_GPU_7Z_STAGE_CRC);
  if ((r = queue_filters(p, g.src.p, filt_x86, filt_arm)) != SZ_OK ||
      (r = split_bcj2(p, bcj2, g.src.p, limit)) != SZ_OK)
    return r;
  mark(LZMA_GPU_7Z_STAGE_FILTER);

  // pieces and first-round slots, in folder order; a BCJ2 folder has four pack
  // streams, each a "folder" of the pack stage
  const size_t nf = p.folders.size();
  std::vector<uint32_t> pack_first(nf);
  uint32_t n_pack = 0;
  size_t next_bcj2 = 0;
  std::vector<SzGpuPackPiece> pieces;
  pieces.reserve(size_t(p.n_pieces));
  std::vector<uint64_t> piece_cap;  // what each piece can add to the pack area
  piece_cap.reserve(size_t(p.n_pieces));
  KindBatch<LzmaEncGpuStreamDesc> lz, l2;
  KindBatch<Ppmd7GpuEncDesc> pp;
  uint64_t at = 0;
  for (size_t k = 0; k < nf; ++k) {
    const FolderPlan& f = p.folders[k];
    const Method& m = p.methods[f.method];
    SzGpuPackPiece pc;
    memset(&pc, 0, sizeof(pc));
    pack_first[k] = n_pack;
    pc.folder = n_pack++;
    if (m.filter == kFilterBcj2) {
      const Bcj2Split& b = bcj2[next_bcj2++];
      n_pack += 3;
      // main, rc, call, jump: the split's streams main, rc, call, jump
      static const int kStream[4] = {LZMA_GPU_BCJ2_MAIN, LZMA_GPU_BCJ2_RC, LZMA_GPU_BCJ2_CALL,
                                     LZMA_GPU_BCJ2_JUMP};
      for (int j = 0; j < 4; ++j) {
        const int sidx = kStream[j];
        pc.folder = pack_first[k] + uint32_t(j);
        if (sidx == LZMA_GPU_BCJ2_RC) {
          pc.kind = LZMA_GPU_7Z_PACK_COPY;
          pc.base = 0;
          pc.off = b.off[sidx];
          pc.len = b.len[sidx];
          pc.slot = 0;
          pieces.push_back(pc);
          piece_cap.push_back(pc.len);
          continue;
        }
        LzmaEncGpuStreamDesc d = sidx == LZMA_GPU_BCJ2_MAIN ? m.proto : m.target_proto;
        d.src_off = b.off[sidx];
        d.src_len = b.len[sidx];
        d.dst_off = at;
        d.dst_cap = first_slot(d.src_len);
        at += d.dst_cap;
        pc.kind = LZMA_GPU_7Z_PACK_LZMA;
        pc.base = 1;
        pc.off = d.dst_off;
        pc.len = 0;
        lz.d.push_back(d);
        lz.piece.push_back(uint32_t(pieces.size()));
        pieces.push_back(pc);
        piece_cap.push_back(d.dst_cap);
      }
    } else if (m.id == kCopy) {
      pc.kind = LZMA_GPU_7Z_PACK_COPY;
      pc.base = 0;
      pc.off = f.off;
      pc.len = f.size;
      pieces.push_back(pc);
      piece_cap.push_back(f.size);
    } else if (m.id == kLzma2) {
      const uint64_t b = lzma2_block(m, f.size);
      for (uint64_t o = 0; o < f.size; o += b) {
        LzmaEncGpuStreamDesc d = m.proto;
        d.src_off = f.off + o;
        d.src_len = std::min<uint64_t>(b, f.size - o);
        d.dst_off = at;
        d.dst_cap = Lzma2EncGpu_BlockBound(size_t(d.src_len));
        at += d.dst_cap;
        pc.kind = LZMA_GPU_7Z_PACK_LZMA2;
        pc.base = 1;
        pc.off = d.dst_off;
        pc.flags = o + b >= f.size ? LZMA_GPU_7Z_PACK_LAST : 0;
        l2.d.push_back(d);
        l2.piece.push_back(uint32_t(pieces.size()));
        pieces.push_back(pc);
        piece_cap.push_back(d.dst_cap + (pc.flags ? 1 : 0));
      }
    } else if (m.id == kLzma) {
      LzmaEncGpuStreamDesc d = m.proto;
      d.src_off = f.off;
      d.src_len = f.size;
      d.dst_off = at;
      d.dst_cap = first_slot(f.size);
      at += d.dst_cap;
      pc.kind = LZMA_GPU_7Z_PACK_LZMA;
      pc.base = 1;
      pc.off = d.dst_off;
      lz.d.push_back(d);
      lz.piece.push_back(uint32_t(pieces.size()));
      pieces.push_back(pc);
      piece_cap.push_back(d.dst_cap);
    } else {
      Ppmd7GpuEncDesc d;
      memset(&d, 0, sizeof(d));
      d.src_off = f.off;
      d.src_len = f.size;
      d.dst_off = at;
      d.dst_cap = first_slot(f.size);
      d.mem_size = m.mem;
      d.order = m.order;
      at += d.dst_cap;
      pc.kind = LZMA_GPU_7Z_PACK_PPMD;
      pc.base = 1;
      pc.off = d.dst_off;
      pp.d.push_back(d);
      pp.piece.push_back(uint32_t(pieces.size()));
      pieces.push_back(pc);
      piece_cap.push_back(d.dst_cap);
    }
  }
  if ((r = lay_out(lz, limit, lzmaenc_slice_bytes)) != SZ_OK || (r = lay_out(l2, limit, lzma2enc_slice_bytes)) != SZ_OK ||
      (r = lay_out(pp, limit, ppmd_slice)) != SZ_OK)
    return r;
  for (size_t k = 0; k < lz.d.size(); ++k) pieces[lz.piece[k]].slot = uint32_t(k);
  for (size_t k = 0; k < l2.d.size(); ++k) pieces[l2.piece[k]].slot = uint32_t(k);
  for (size_t k = 0; k < pp.d.size(); ++k) pieces[pp.piece[k]].slot = uint32_t(k);

  g.ws_bytes = std::max(lz.plan.ws_max, std::max(l2.plan.ws_max, pp.plan.ws_max));
  const size_t lz_cap = lz.d.size() * (1 + kReencodeRounds);
  const size_t pp_cap = pp.d.size() * (1 + kReencodeRounds);
  if ((r = alloc_all("7z write", g.slots, size_t(at), g.ws, size_t(g.ws_bytes), g.lz_res, lz_cap,
                     g.l2_res, l2.d.size(), g.pp_res, pp_cap)) != SZ_OK)
    return r;
  DevArr<LzmaEncGpuStreamDesc> g_lz, g_l2;
  DevArr<Ppmd7GpuEncDesc> g_pp;
  if ((r = launch_lzma(lz, g_lz, g.src.p, g.slots.p, g.ws.p, g.lz_res.p, &st.encode_launches)) !=
          SZ_OK ||
      (r = launch_lzma2(l2, g_l2, g.src.p, g.slots.p, g.ws.p, g.l2_res.p, &st.encode_launches)) !=
          SZ_OK ||
      (r = launch_ppmd(pp, g_pp, g.src.p, g.slots.p, g.ws.p, g.pp_res.p, &st.encode_launches)) !=
          SZ_OK)
    return r;

  // the streams that did not fit their slot, again with a larger one
  size_t lz_used = lz.d.size(), pp_used = pp.d.size();
  KindBatch<LzmaEncGpuStreamDesc> lz_cur;
  KindBatch<Ppmd7GpuEncDesc> pp_cur;
  lz_cur.d = lz.d;
  lz_cur.piece = lz.piece;
  pp_cur.d = pp.d;
  pp_cur.piece = pp.piece;
  size_t lz_at = 0, pp_at = 0;  // where the current round's results start
  DevArr<LzmaEncGpuStreamDesc> g_lz_retry[kReencodeRounds];
  DevArr<Ppmd7GpuEncDesc> g_pp_retry[kReencodeRounds];
  for (unsigned round = 1;; ++round) {
    std::vector<LzmaEncGpuResult> lr(lz_cur.d.size());
    std::vector<Ppmd7GpuEncResult> pr(pp_cur.d.size());
    if (!hip_ok(hipDeviceSynchronize(), "7z write: encode") ||
        (!lr.empty() && !hip_ok(hipMemcpy(lr.data(), g.lz_res.p + lz_at, lr.size() * sizeof(lr[0]),
                                          hipMemcpyDeviceToHost), "download results")) ||
        (!pr.empty() && !hip_ok(hipMemcpy(pr.data(), g.pp_res.p + pp_at, pr.size() * sizeof(pr[0]),
                                          hipMemcpyDeviceToHost), "download results")))
      return SZ_ERROR_FAIL;
    KindBatch<LzmaEncGpuStreamDesc> lz_next;
    KindBatch<Ppmd7GpuEncDesc> pp_next;
    uint64_t need = 0;
    for (size_t k = 0; k < lr.size(); ++k) {
      if (lr[k].res != SZ_ERROR_OUTPUT_EOF) continue;
      LzmaEncGpuStreamDesc d = lz_cur.d[k];
      d.dst_off = need;
      d.dst_cap = lzma_retry_slot(d.src_len, round);
      need += d.dst_cap;
      lz_next.d.push_back(d);
      lz_next.piece.push_back(lz_cur.piece[k]);
    }
    for (size_t k = 0; k < pr.size(); ++k) {
      if (pr[k].res != SZ_ERROR_OUTPUT_EOF) continue;
      Ppmd7GpuEncDesc d = pp_cur.d[k];
      d.dst_off = need;
      d.dst_cap = pr[k].packed_len;
      need += d.dst_cap;
      pp_next.d.push_back(d);
      pp_next.piece.push_back(pp_cur.piece[k]);
    }
    if (lz_next.d.empty() && pp_next.d.empty()) break;
    if (round > kReencodeRounds) {
      set_error("7z write: a stream did not fit its slot after two larger ones");
      return SZ_ERROR_FAIL;
    }
    // the workspace stands: cut by its size (every slice fitted it before)
    if ((r = lay_out(lz_next, g.ws_bytes, lzmaenc_slice_bytes)) != SZ_OK ||
        (r = lay_out(pp_next, g.ws_bytes, ppmd_slice)) != SZ_OK)
      return r;
    if ((r = alloc_all("7z write", g.retry[round - 1], size_t(need))) != SZ_OK) return r;
    lz_at = lz_used;
    pp_at = pp_used;
    for (size_t k = 0; k < lz_next.d.size(); ++k) {
      SzGpuPackPiece& pc = pieces[lz_next.piece[k]];
      pc.base = uint16_t(1 + round);
      pc.off = lz_next.d[k].dst_off;
      pc.slot = uint32_t(lz_at + k);
      piece_cap[lz_next.piece[k]] = lz_next.d[k].dst_cap;
    }
    for (size_t k = 0; k < pp_next.d.size(); ++k) {
      SzGpuPackPiece& pc = pieces[pp_next.piece[k]];
      pc.base = uint16_t(1 + round);
      pc.off = pp_next.d[k].dst_off;
      pc.slot = uint32_t(pp_at + k);
      piece_cap[pp_next.piece[k]] = pp_next.d[k].dst_cap;
    }
    lz_used += lz_next.d.size();
    pp_used += pp_next.d.size();
    st.reencoded += lz_next.d.size() + pp_next.d.size();
    uint8_t* area = g.retry[round - 1].p;
    if ((r = launch_lzma(lz_next, g_lz_retry[round - 1], g.src.p, area, g.ws.p,
                         g.lz_res.p + lz_at, &st.encode_launches)) != SZ_OK ||
        (r = launch_ppmd(pp_next, g_pp_retry[round - 1], g.src.p, area, g.ws.p,
                         g.pp_res.p + pp_at, &st.encode_launches)) != SZ_OK)
      return r;
    lz_cur.d.swap(lz_next.d);
    lz_cur.piece.swap(lz_next.piece);
    pp_cur.d.swap(pp_next.d);
    pp_cur.piece.swap(pp_next.piece);
  }

  mark(LZMA_GPU_7Z_STAGE_ENCODE);

  // pack
  uint64_t out_cap = 0;
  for (uint64_t c : piece_cap) out_cap += c;
  const size_t np = pieces.size();
  DevArr<SzGpuPackPiece> g_pieces;
  DevArr<uint64_t> g_scratch, g_off, g_fsize;
  DevArr<LzmaEncGpuResult> g_total;
  if ((r = upload(g_pieces, pieces, "7z write")) != SZ_OK ||
      (r = alloc_all("7z write", g.out, size_t(out_cap), g_scratch, SzGpu_PackScratch(np), g_off,
                     np, g_fsize, n_pack, g_total, 1)) != SZ_OK)
    return r;
  SzGpuPackArgs a;
  memset(&a, 0, sizeof(a));
  a.d_pieces = g_pieces.p;
  a.n = np;
  a.n_folders = n_pack;
  a.bases[0] = g.src.p;
  a.bases[1] = g.slots.p;
  for (unsigned k = 0; k < kReencodeRounds; ++k) a.bases[2 + k] = g.retry[k].p;
  a.d_lzma = g.lz_res.p;
  a.n_lzma = lz_used;
  a.d_lzma2 = g.l2_res.p;
  a.n_lzma2 = l2.d.size();
  a.d_ppmd = g.pp_res.p;
  a.n_ppmd = pp_used;
  a.d_out = g.out.p;
  a.out_cap = out_cap;
  a.d_scratch = g_scratch.p;
  a.d_piece_off = g_off.p;
  a.d_folder_size = g_fsize.p;
  a.d_total = g_total.p;
  if (szpackgpu_launch(&a, nullptr) != 0) {
    set_error("7z write: pack launch failed");
    return SZ_ERROR_FAIL;
  }
  LzmaEncGpuResult total;
  std::vector<uint64_t> fsize(n_pack);
  std::vector<uint32_t> crcs(crc.n);
  if (!hip_ok(hipDeviceSynchronize(), "7z write: pack") ||
      !hip_ok(hipMemcpy(&total, g_total.p, sizeof(total), hipMemcpyDeviceToHost),
              "download total"))
    return SZ_ERROR_FAIL;
  mark(LZMA_GPU_7Z_STAGE_PACK);
  if (total.res != SZ_OK) {  // slots of the block bound fit; the rest fitted above
    set_error("7z write: a piece failed on the device");
    return SZ_ERROR_FAIL;
  }
  if ((n_pack && !hip_ok(hipMemcpy(fsize.data(), g_fsize.p, n_pack * 8, hipMemcpyDeviceToHost),
                     "download pack sizes")) ||
      !crc.fetch(crcs.data(), "download CRCs"))
    return SZ_ERROR_FAIL;

  // header
  std::vector<LzmaGpu7zFolder> folders(nf);
  for (size_t k = 0; k < nf; ++k) {
    fill_folder(p, k, folders[k]);
    folders[k].pack_size = fsize[pack_first[k]];
  }
  std::vector<LzmaGpu7zBcj2Info> infos(bcj2.size());
  for (size_t i = 0; i < bcj2.size(); ++i) {
    const Bcj2Split& b = bcj2[i];
    const Method& m = p.methods[p.folders[b.folder].method];
    LzmaGpu7zBcj2Info& o = infos[i];
    memset(&o, 0, sizeof(o));
    for (int j = 0; j < 4; ++j) o.pack_size[j] = fsize[pack_first[b.folder] + j];
    o.unpack_size[0] = b.len[LZMA_GPU_BCJ2_JUMP];
    o.unpack_size[1] = b.len[LZMA_GPU_BCJ2_CALL];
    o.unpack_size[2] = b.len[LZMA_GPU_BCJ2_MAIN];
    memcpy(o.call_props, m.target_props, 5);
    memcpy(o.jump_props, m.target_props, 5);
  }
  std::vector<uint32_t> file_crcs(n, 0);
  for (size_t i = 0, d = 0; i < n; ++i)
    if (has_data(items[i])) file_crcs[i] = crcs[d++];
  Bytes hdr, hpack;
  if ((r = build_header(folders.data(), nf, items, n, file_crcs.data(), names, names_len, hdr,
                        infos.data(), infos.size())) != SZ_OK)
    return r;
  const uint64_t pack_total = total.dest_len;
  if (flags & LZMA_GPU_7Z_WRITE_ENCODE_HEADER) {
    LzmaGpu7zFolder hf;
    memset(&hf, 0, sizeof(hf));
    if ((r = encode_header_stream(hdr, hpack, hf.props)) != SZ_OK) return r;
    hf.pack_off = pack_total;
    hf.pack_size = hpack.size();
    hf.unpack_size = hdr.size();
    hf.method = kLzma;
    hf.crc_defined = 1;
    hf.crc = crc32_host(hdr.data(), hdr.size());
    hf.num_files = 1;
    hf.num_coders = 1;
    hf.props_size = 5;
    Bytes stub;
    if ((r = build_stub(&hf, 1, stub)) != SZ_OK) return r;
    hdr.swap(stub);
  }
  mark(LZMA_GPU_7Z_STAGE_HEADER);
  const uint64_t need = 32 + pack_total + hpack.size() + hdr.size();
  st.folders = nf;
  st.pieces = np;
  st.pack_bytes = pack_total + hpack.size();
  st.header_bytes = hdr.size();
  if (stats) *stats = st;
  if (need > *destLen) {
    *destLen = SizeT(need);
    return SZ_ERROR_OUTPUT_EOF;
  }
  if (pack_total && !hip_ok(hipMemcpy(dest + 32, g.out.p, size_t(pack_total),
                                      hipMemcpyDeviceToHost), "download pack area"))
    return SZ_ERROR_FAIL;
  if (!hpack.empty()) memcpy(dest + 32 + pack_total, hpack.data(), hpack.size());
  memcpy(dest + 32 + pack_total + hpack.size(), hdr.data(), hdr.size());
  write_sig(dest, hdr, pack_total + hpack.size());
  *destLen = SizeT(need);
  mark(LZMA_GPU_7Z_STAGE_DOWNLOAD);
  st.stage_ns[LZMA_GPU_7Z_STAGE_TOTAL] = uint64_t(
      std::chrono::nanoseconds(std::chrono::steady_clock::now() - t_begin).count());
  if (stats) *stats = st;
  return SZ_OK;
}

}  // namespace

extern "C" SRes LzmaGpu_7zWritePlan(const LzmaGpu7zItem* items, size_t n, size_t src_size,
                                    size_t names_len, const LzmaGpu7zMethod* methods,
                                    size_t n_methods, LzmaGpu7zFolder* folders, size_t folder_cap,
                                    size_t* n_folders, size_t* n_pieces, uint64_t* dest_bound) {
  return guarded("7z write: host allocation failed", [&]() -> SRes {
    Plan p;
    const SRes r = make_plan(items, n, src_size, names_len, methods, n_methods, p);
    if (r != SZ_OK) return r;
    if (n_folders) *n_folders = p.folders.size();
    if (n_pieces) *n_pieces = size_t(p.n_pieces);
    if (dest_bound) {
      const uint64_t hb = header_bound(p.folders.size(), size_t(p.n_bcj2), n, names_len);
      *dest_bound = 32 + p.pack_bound + lzma_retry_slot(hb, kReencodeRounds) + hb + 64;
    }
    for (size_t k = 0; folders && k < p.folders.size() && k < folder_cap; ++k)
      fill_folder(p, k, folders[k]);
    return SZ_OK;
  });
}

extern "C" SRes LzmaGpu_7zWriteHeaderEx(const LzmaGpu7zFolder* folders, size_t n_folders,
                                        const LzmaGpu7zItem* items, size_t n,
                                        const uint32_t* file_crcs, const UInt16* names,
                                        size_t names_len, unsigned flags,
                                        const LzmaGpu7zBcj2Info* bcj2, size_t n_bcj2, Byte* header,
                                        size_t header_cap, size_t* header_len, Byte* sig32,
                                        uint64_t pack_area_size) {
  return guarded("7z write: host allocation failed", [&]() -> SRes {
    if (flags & ~unsigned(LZMA_GPU_7Z_HEADER_STUB)) return SZ_ERROR_PARAM;
    Bytes o;
    const SRes r = (flags & LZMA_GPU_7Z_HEADER_STUB)
                       ? build_stub(folders, n_folders, o)
                       : build_header(folders, n_folders, items, n, file_crcs, names, names_len, o,
                                      bcj2, n_bcj2);
    if (r != SZ_OK) return r;
    if (header_len) *header_len = o.size();
    if (sig32) write_sig(sig32, o, pack_area_size);
    if (!header || header_cap < o.size()) return SZ_ERROR_OUTPUT_EOF;
    memcpy(header, o.data(), o.size());
    return SZ_OK;
  });
}

extern "C" SRes LzmaGpu_7zWriteHeader(const LzmaGpu7zFolder* folders, size_t n_folders,
                                      const LzmaGpu7zItem* items, size_t n,
                                      const uint32_t* file_crcs, const UInt16* names,
                                      size_t names_len, unsigned flags, Byte* header,
                                      size_t header_cap, size_t* header_len, Byte* sig32,
                                      uint64_t pack_area_size) {
  return LzmaGpu_7zWriteHeaderEx(folders, n_folders, items, n, file_crcs, names, names_len, flags,
                                 nullptr, 0, header, header_cap, header_len, sig32,
                                 pack_area_size);
}

extern "C" SRes LzmaGpu_7zWrite(Byte* dest, SizeT* destLen, const Byte* src, size_t src_size,
                                const LzmaGpu7zItem* items, size_t n, const UInt16* names,
                                size_t names_len, const LzmaGpu7zMethod* methods, size_t n_methods,
                                const LzmaGpu7zWriteOptions* options, LzmaGpu7zWriteStats* stats) {
  return guarded("7z write: host allocation failed", [&]() {
    return write_archive(dest, destLen, src, src_size, items, n, names, names_len, methods,
                         n_methods, options, stats);
  });
}

extern "C" size_t SzGpu_PackScratch(size_t n) { return size_t(szpack::scratch_words(n)); }

extern "C" SRes SzGpu_PackBatch(const SzGpuPackArgs* args, void* stream) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  if (args->n > 0x7FFFFFFFull) return SZ_ERROR_PARAM;
  if (szpackgpu_launch(args, static_cast<hipStream_t>(stream)) != 0) {
    set_error("7z pack kernel launch failed");
    return SZ_ERROR_FAIL;
  }
  return SZ_OK;
}
