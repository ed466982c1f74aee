// sevenz_capi.hip -- 7z archives as GPU folder batches (include/lzma_gpu.h,
// SURVEY.md 8(f) row 3).
//
// The reference opens an archive with SzArEx_Open (7zIn.c:1214-1320: start
// header, next header, an optional packed header decoded through a folder)
// and extracts file by file with SzArEx_Extract (7zIn.c:1322-1402), which
// decodes the file's whole folder (SzFolder_Decode, 7zDec.c:335-471) into a
// cached buffer and checks the folder and file CRCs.  Here the header walk
// is restated on the host (it is a few hundred bytes of metadata), and every
// folder of the archive becomes one item of a single GPU batch: LZMA / LZMA2
// main coders through LzmaGpu_PlanBatchEx / LzmaGpu_DecodeBatchEx, Copy
// folders as device copies, then the x86 BCJ kernel over BCJ folders and one
// CRC-32 batch over every folder and file range.  Per-file results are what
// SzArEx_Extract returns for that file with a fresh folder cache.
//
// PPMd (method 0x030401, SzDecodePpmd 7zDec.c:29-124) is a compile-time switch
// of the reference (_7ZIP_PPMD_SUPPPORT) and a run-time flag here
// (LZMA_GPU_7Z_PPMD of the Ex entry points; off = the reference as built):
// its coders run as one Ppmd7Gpu_DecodeBatch beside the LZMA batch.  Deviation
// from the reference's switch: a PPMd coder inside a BCJ2 folder stays
// SZ_ERROR_UNSUPPORTED with the flag.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include "host_batch.h"
#include "lzma_gpu_internal.h"
#include "ppmd7_internal.h"

using namespace lzgpu_host;

namespace {

// property ids (7z.h:17-45)
enum : uint64_t {
  kEnd = 0, kHeader, kArchiveProperties, kAdditionalStreamsInfo, kMainStreamsInfo, kFilesInfo,
  kPackInfo, kUnpackInfo, kSubStreamsInfo, kSize, kCRC, kFolder, kCodersUnpackSize,
  kNumUnpackStream, kEmptyStream, kEmptyFile, kAnti, kName, kCTime, kATime, kMTime,
  kWinAttributes, kComment, kEncodedHeader
};
// coder ids (7zDec.c:19-31)
constexpr uint64_t kCopy = 0, kLzma = 0x30101, kLzma2 = 0x21, kBcj = 0x03030103,
                   kArm = 0x03030501, kBcj2 = 0x0303011B, kPpmd = 0x30401;
constexpr size_t kStartHeader = 32;
constexpr uint32_t kNoFolder = 0xFFFFFFFFu;

#define RINOK7(x)                  \
  do {                             \
    const SRes r_ = (x);           \
    if (r_ != SZ_OK) return r_;    \
  } while (0)

struct Coder {
  uint64_t method = 0;
  uint32_t nin = 1, nout = 1;
  std::vector<Byte> props;
};
struct BindPair {
  uint32_t in = 0, out = 0;
};
struct Folder {
  std::vector<Coder> coders;
  std::vector<BindPair> bind;
  std::vector<uint32_t> pack_streams;
  std::vector<uint64_t> unpack_sizes;
  bool crc_defined = false;
  uint32_t crc = 0;
  uint32_t num_unpack_streams = 0;  // SzFolder_Init: 1 only once a SubStreamsInfo is read
  uint32_t num_out() const {
    uint32_t n = 0;
    for (const Coder& c : coders) n += c.nout;
    return n;
  }
  bool bound_in(uint32_t i) const {
    for (const BindPair& b : bind)
      if (b.in == i) return true;
    return false;
  }
  bool bound_out(uint32_t i) const {
    for (const BindPair& b : bind)
      if (b.out == i) return true;
    return false;
  }
  // SzFolder_GetUnpackSize (7zIn.c:83-93): the one out stream nothing binds
  uint64_t unpack_size() const {
    for (int i = int(num_out()) - 1; i >= 0; --i)
      if (!bound_out(uint32_t(i))) return i < int(unpack_sizes.size()) ? unpack_sizes[i] : 0;
    return 0;
  }
};
struct Ar {
  std::vector<uint64_t> pack_sizes;
  std::vector<Folder> folders;
  uint64_t data_pos = 0;
};
struct SubStreams {
  uint32_t n = 0;
  std::vector<uint64_t> sizes;
  std::vector<Byte> defined;
  std::vector<uint32_t> digests;
};
struct FileItem {
  bool has_stream = true, is_dir = false;
  uint64_t size = 0;
  uint32_t crc = 0;
  bool crc_defined = false;
};
struct Archive {
  Ar db;
  std::vector<FileItem> files;
  std::vector<Byte> names;           // FileNames: UTF-16LE
  std::vector<size_t> name_offsets;  // FileNameOffsets (UTF-16 units), numFiles + 1
  std::vector<uint32_t> folder_start_pack, folder_start_file, file_folder;
  std::vector<uint64_t> pack_start;
  unsigned flags = 0;  // LZMA_GPU_7Z_*
};

// CSzData readers (7zIn.c:310-400)
struct Sd {
  const Byte* p;
  size_t n;
};
SRes rd_byte(Sd& s, Byte* b) {
  if (s.n == 0) return SZ_ERROR_ARCHIVE;
  --s.n;
  *b = *s.p++;
  return SZ_OK;
}
SRes rd_bytes(Sd& s, Byte* d, size_t k) {
  for (size_t i = 0; i < k; ++i) RINOK7(rd_byte(s, d + i));
  return SZ_OK;
}
SRes rd_u32(Sd& s, uint32_t* v) {
  *v = 0;
  for (int i = 0; i < 4; ++i) {
    Byte b;
    RINOK7(rd_byte(s, &b));
    *v |= uint32_t(b) << (8 * i);
  }
  return SZ_OK;
}
// SzReadNumber: leading one bits of the first byte = extra bytes
SRes rd_num(Sd& s, uint64_t* v) {
  Byte first, mask = 0x80;
  RINOK7(rd_byte(s, &first));
  *v = 0;
  for (int i = 0; i < 8; ++i) {
    if ((first & mask) == 0) {
      *v += uint64_t(first & (mask - 1)) << (8 * i);
      return SZ_OK;
    }
    Byte b;
    RINOK7(rd_byte(s, &b));
    *v |= uint64_t(b) << (8 * i);
    mask >>= 1;
  }
  return SZ_OK;
}
SRes rd_num32(Sd& s, uint32_t* v) {
  uint64_t x;
  RINOK7(rd_num(s, &x));
  if (x >= 0x80000000ull) return SZ_ERROR_UNSUPPORTED;
  *v = uint32_t(x);
  return SZ_OK;
}
SRes skip_size(Sd& s, uint64_t size) {
  if (size > s.n) return SZ_ERROR_ARCHIVE;
  s.n -= size_t(size);
  s.p += size_t(size);
  return SZ_OK;
}
SRes skip_data(Sd& s) {
  uint64_t size;
  RINOK7(rd_num(s, &size));
  return skip_size(s, size);
}
SRes wait_attr(Sd& s, uint64_t attr) {
  for (;;) {
    uint64_t t;
    RINOK7(rd_num(s, &t));
    if (t == attr) return SZ_OK;
    if (t == kEnd) return SZ_ERROR_ARCHIVE;
    RINOK7(skip_data(s));
  }
}
SRes bool_vec(Sd& s, size_t n, std::vector<Byte>* v) {
  v->assign(n, 0);
  Byte b = 0, mask = 0;
  for (size_t i = 0; i < n; ++i) {
    if (mask == 0) {
      RINOK7(rd_byte(s, &b));
      mask = 0x80;
    }
    (*v)[i] = (b & mask) ? 1 : 0;
    mask >>= 1;
  }
  return SZ_OK;
}
SRes bool_vec2(Sd& s, size_t n, std::vector<Byte>* v) {
  Byte all;
  RINOK7(rd_byte(s, &all));
  if (all == 0) return bool_vec(s, n, v);
  v->assign(n, 1);
  return SZ_OK;
}
SRes hash_digests(Sd& s, size_t n, std::vector<Byte>* defined, std::vector<uint32_t>* digests) {
  RINOK7(bool_vec2(s, n, defined));
  digests->assign(n, 0);
  for (size_t i = 0; i < n; ++i)
    if ((*defined)[i]) RINOK7(rd_u32(s, &(*digests)[i]));
  return SZ_OK;
}
SRes rd_switch(Sd& s) {
  Byte external;
  RINOK7(rd_byte(s, &external));
  return external == 0 ? SZ_OK : SZ_ERROR_UNSUPPORTED;
}

// SzReadPackInfo (7zIn.c:481-527)
SRes read_pack_info(Sd& s, uint64_t* data_offset, Ar& a) {
  uint32_t n;
  RINOK7(rd_num(s, data_offset));
  RINOK7(rd_num32(s, &n));
  RINOK7(wait_attr(s, kSize));
  // every pack size takes >= 1 header byte: a count beyond the bytes left
  // cannot be read (the reference's MY_ALLOC would ask for n * 8 bytes first)
  if (n > s.n) return SZ_ERROR_ARCHIVE;
  a.pack_sizes.assign(n, 0);
  for (uint32_t i = 0; i < n; ++i) RINOK7(rd_num(s, &a.pack_sizes[i]));
  for (;;) {
    uint64_t t;
    RINOK7(rd_num(s, &t));
    if (t == kEnd) break;
    if (t == kCRC) {
      std::vector<Byte> d;
      std::vector<uint32_t> c;
      RINOK7(hash_digests(s, n, &d, &c));  // pack CRCs: read, never checked by the reader
      continue;
    }
    RINOK7(skip_data(s));
  }
  return SZ_OK;
}

// SzGetNextFolderItem (7zIn.c:536-644)
SRes next_folder(Sd& s, Folder& f) {
  uint32_t nc, n_in = 0, n_out = 0;
  RINOK7(rd_num32(s, &nc));
  if (nc > 32) return SZ_ERROR_UNSUPPORTED;
  f.coders.assign(nc, Coder());
  for (uint32_t i = 0; i < nc; ++i) {
    Coder& c = f.coders[i];
    Byte main;
    RINOK7(rd_byte(s, &main));
    const unsigned id_size = main & 0xF;
    Byte id[15];
    RINOK7(rd_bytes(s, id, id_size));
    if (id_size > 8) return SZ_ERROR_UNSUPPORTED;
    c.method = 0;
    for (unsigned j = 0; j < id_size; ++j) c.method |= uint64_t(id[id_size - 1 - j]) << (8 * j);
    if (main & 0x10) {
      RINOK7(rd_num32(s, &c.nin));
      RINOK7(rd_num32(s, &c.nout));
      if (c.nin > 32 || c.nout > 32) return SZ_ERROR_UNSUPPORTED;
    }
    if (main & 0x20) {
      uint64_t ps;
      RINOK7(rd_num(s, &ps));
      if (ps > s.n) return SZ_ERROR_ARCHIVE;
      c.props.resize(size_t(ps));
      RINOK7(rd_bytes(s, c.props.data(), size_t(ps)));
    }
    while (main & 0x80) {  // alternative methods: skipped
      RINOK7(rd_byte(s, &main));
      RINOK7(skip_size(s, main & 0xF));
      if (main & 0x10) {
        uint32_t x;
        RINOK7(rd_num32(s, &x));
        RINOK7(rd_num32(s, &x));
      }
      if (main & 0x20) {
        uint64_t ps;
        RINOK7(rd_num(s, &ps));
        RINOK7(skip_size(s, ps));
      }
    }
    n_in += c.nin;
    n_out += c.nout;
  }
  if (n_out == 0) return SZ_ERROR_UNSUPPORTED;
  f.bind.assign(n_out - 1, BindPair());
  for (BindPair& b : f.bind) {
    RINOK7(rd_num32(s, &b.in));
    RINOK7(rd_num32(s, &b.out));
  }
  if (n_in < f.bind.size()) return SZ_ERROR_UNSUPPORTED;
  const uint32_t np = n_in - uint32_t(f.bind.size());
  f.pack_streams.assign(np, 0);
  if (np == 1) {
    uint32_t i = 0;
    while (i < n_in && f.bound_in(i)) ++i;
    if (i == n_in) return SZ_ERROR_UNSUPPORTED;
    f.pack_streams[0] = i;
  } else {
    for (uint32_t i = 0; i < np; ++i) RINOK7(rd_num32(s, &f.pack_streams[i]));
  }
  return SZ_OK;
}

// SzReadUnpackInfo (7zIn.c:646-714)
SRes read_unpack_info(Sd& s, Ar& a) {
  uint32_t nf;
  RINOK7(wait_attr(s, kFolder));
  RINOK7(rd_num32(s, &nf));
  RINOK7(rd_switch(s));
  if (nf > s.n) return SZ_ERROR_ARCHIVE;  // a folder takes >= 1 header byte
  a.folders.assign(nf, Folder());
  for (uint32_t i = 0; i < nf; ++i) RINOK7(next_folder(s, a.folders[i]));
  RINOK7(wait_attr(s, kCodersUnpackSize));
  for (Folder& f : a.folders) {
    f.unpack_sizes.assign(f.num_out(), 0);
    for (uint64_t& u : f.unpack_sizes) RINOK7(rd_num(s, &u));
  }
  for (;;) {
    uint64_t t;
    RINOK7(rd_num(s, &t));
    if (t == kEnd) return SZ_OK;
    if (t == kCRC) {
      std::vector<Byte> d;
      std::vector<uint32_t> c;
      RINOK7(hash_digests(s, nf, &d, &c));
      for (uint32_t i = 0; i < nf; ++i) {
        a.folders[i].crc_defined = d[i] != 0;
        a.folders[i].crc = c[i];
      }
      continue;
    }
    RINOK7(skip_data(s));
  }
}

// SzReadSubStreamsInfo (7zIn.c:716-860)
SRes read_substreams(Sd& s, Ar& a, SubStreams& ss) {
  uint64_t t = 0;
  for (Folder& f : a.folders) f.num_unpack_streams = 1;
  ss.n = uint32_t(a.folders.size());
  for (;;) {
    RINOK7(rd_num(s, &t));
    if (t == kNumUnpackStream) {
      ss.n = 0;
      for (Folder& f : a.folders) {
        RINOK7(rd_num32(s, &f.num_unpack_streams));
        ss.n += f.num_unpack_streams;
      }
      continue;
    }
    if (t == kCRC || t == kSize || t == kEnd) break;
    RINOK7(skip_data(s));
  }
  // With a kSize section a folder's substreams after its first each need a
  // size (>= 1 header byte): more than that cannot be described by the bytes
  // left.  Without one the reference takes any count it can allocate (sizes
  // of all but a folder's last substream stay unset there, 7zIn.c:757-768).
  // DELIBERATE DEVIATION: counts past 2^24 return
  // SZ_ERROR_MEM here instead of being attempted -- 2^31 substreams would zero
  // 28 GB of host memory before failing or succeeding, which a library call
  // on behalf of an untrusted header must not do.  Below the cap an
  // allocation failure is reported the same way.
  if (t == kSize && uint64_t(ss.n) > uint64_t(s.n) + a.folders.size()) return SZ_ERROR_ARCHIVE;
  if (ss.n > (1u << 24)) return SZ_ERROR_MEM;
  try {
    ss.sizes.assign(ss.n, 0);
    ss.defined.assign(ss.n, 0);
    ss.digests.assign(ss.n, 0);
  } catch (const std::bad_alloc&) {
    return SZ_ERROR_MEM;
  }
  uint32_t si = 0;
  for (Folder& f : a.folders) {
    const uint32_t k = f.num_unpack_streams;
    if (k == 0) continue;
    uint64_t sum = 0;
    if (t == kSize)
      for (uint32_t j = 1; j < k; ++j) {
        uint64_t size;
        RINOK7(rd_num(s, &size));
        if (si < ss.n) ss.sizes[si] = size;
        ++si;
        sum += size;
      }
    if (si < ss.n) ss.sizes[si] = f.unpack_size() - sum;
    ++si;
  }
  if (t == kSize) RINOK7(rd_num(s, &t));
  uint32_t n_digests = 0;
  for (const Folder& f : a.folders)
    if (f.num_unpack_streams != 1 || !f.crc_defined) n_digests += f.num_unpack_streams;
  si = 0;
  bool have_crc = false;
  for (;;) {
    if (t == kCRC) {
      // a second kCRC section: the reference goes on writing behind its digest
      // arrays (si is not reset, 7zIn.c:814-843)
      if (have_crc && ss.n != 0) return SZ_ERROR_ARCHIVE;
      have_crc = true;
      std::vector<Byte> d2;
      std::vector<uint32_t> c2;
      RINOK7(hash_digests(s, n_digests, &d2, &c2));
      size_t di = 0;
      for (const Folder& f : a.folders) {
        if (f.num_unpack_streams == 1 && f.crc_defined) {
          if (si < ss.n) {
            ss.defined[si] = 1;
            ss.digests[si] = f.crc;
          }
          ++si;
        } else {
          for (uint32_t j = 0; j < f.num_unpack_streams; ++j, ++di, ++si)
            if (si < ss.n && di < d2.size()) {
              ss.defined[si] = d2[di];
              ss.digests[si] = c2[di];
            }
        }
      }
    } else if (t == kEnd) {
      return SZ_OK;
    } else {
      RINOK7(skip_data(s));
    }
    RINOK7(rd_num(s, &t));
  }
}

// SzReadStreamsInfo (7zIn.c:862-917)
SRes read_streams_info(Sd& s, uint64_t* data_offset, Ar& a, SubStreams& ss, bool* have_ss) {
  for (;;) {
    uint64_t t;
    RINOK7(rd_num(s, &t));
    if (t > 0x7FFFFFFFull) return SZ_ERROR_UNSUPPORTED;
    switch (t) {
      case kEnd:
        return SZ_OK;
      case kPackInfo:
        RINOK7(read_pack_info(s, data_offset, a));
        break;
      case kUnpackInfo:
        RINOK7(read_unpack_info(s, a));
        break;
      case kSubStreamsInfo:
        RINOK7(read_substreams(s, a, ss));
        *have_ss = true;
        break;
      default:
        return SZ_ERROR_UNSUPPORTED;
    }
  }
}

// SzReadFileNames (7zIn.c:919-938); size in UTF-16 units
SRes read_file_names(const Byte* p, size_t size, uint32_t n, std::vector<size_t>* off) {
  off->assign(size_t(n) + 1, 0);
  size_t pos = 0;
  for (uint32_t i = 0; i < n; ++i) {
    (*off)[i] = pos;
    for (;;) {
      if (pos >= size) return SZ_ERROR_ARCHIVE;
      if (p[pos * 2] == 0 && p[pos * 2 + 1] == 0) break;
      ++pos;
    }
    ++pos;
  }
  (*off)[n] = pos;
  return pos == size ? SZ_OK : SZ_ERROR_ARCHIVE;
}

// SzArEx_Fill (7zIn.c:179-247)
SRes fill(Archive& x) {
  const Ar& a = x.db;
  x.folder_start_pack.assign(a.folders.size(), 0);
  uint32_t sp = 0;
  for (size_t i = 0; i < a.folders.size(); ++i) {
    x.folder_start_pack[i] = sp;
    sp += uint32_t(a.folders[i].pack_streams.size());
  }
  x.pack_start.assign(a.pack_sizes.size(), 0);
  uint64_t pos = 0;
  for (size_t i = 0; i < a.pack_sizes.size(); ++i) {
    x.pack_start[i] = pos;
    pos += a.pack_sizes[i];
  }
  x.folder_start_file.assign(a.folders.size(), 0);
  x.file_folder.assign(x.files.size(), kNoFolder);
  uint32_t fi = 0, in_folder = 0;
  for (size_t i = 0; i < x.files.size(); ++i) {
    const bool empty = !x.files[i].has_stream;
    if (empty && in_folder == 0) continue;
    if (in_folder == 0) {
      for (;;) {
        if (fi >= a.folders.size()) return SZ_ERROR_ARCHIVE;
        x.folder_start_file[fi] = uint32_t(i);
        if (a.folders[fi].num_unpack_streams != 0) break;
        ++fi;
      }
    }
    x.file_folder[i] = fi;
    // the reference decodes this folder for the file and indexes PackSizes
    // unchecked (7zIn.c:1373-1375, 7zDec.c:385-386): a folder that needs more
    // pack sizes than PackInfo gave
    if (uint64_t(x.folder_start_pack[fi]) + a.folders[fi].pack_streams.size() > a.pack_sizes.size())
      return SZ_ERROR_ARCHIVE;
    if (empty) continue;
    if (++in_folder >= a.folders[fi].num_unpack_streams) {
      ++fi;
      in_folder = 0;
    }
  }
  return SZ_OK;
}

// SzReadHeader2 (7zIn.c:940-1120)
SRes read_header(Archive& x, Sd& s) {
  uint64_t t;
  SubStreams ss;
  bool have_ss = false;
  RINOK7(rd_num(s, &t));
  if (t == kArchiveProperties) {
    for (;;) {  // SzReadArchiveProperties: the skip result is not checked there
      uint64_t u;
      RINOK7(rd_num(s, &u));
      if (u == kEnd) break;
      (void)skip_data(s);
    }
    RINOK7(rd_num(s, &t));
  }
  if (t == kMainStreamsInfo) {
    RINOK7(read_streams_info(s, &x.db.data_pos, x.db, ss, &have_ss));
    x.db.data_pos += kStartHeader;
    RINOK7(rd_num(s, &t));
  }
  // no kFilesInfo: folders and no files (7zIn.c:981-982 returns here with its
  // Fill arrays unset and never walks them: no file, no extract); the folder
  // tables the open and extract calls walk are filled all the same
  if (t == kEnd) return fill(x);
  if (t != kFilesInfo) return SZ_ERROR_ARCHIVE;
  uint32_t nf;
  RINOK7(rd_num32(s, &nf));
  // A file with a stream needs no header byte of its own (no name, sizes and
  // CRCs from the substreams: 7zIn.c:986-1104 accepts that); an empty-stream
  // file costs >= 1 bit of the kEmptyStream vector.  A count beyond both is
  // malformed, not allocated.
  if (uint64_t(nf) > 8 * uint64_t(s.n) + 64 + (have_ss ? uint64_t(ss.n) : 0))
    return SZ_ERROR_ARCHIVE;
  x.files.assign(nf, FileItem());
  std::vector<Byte> empty_stream, empty_file, defined;
  uint32_t n_empty = 0;
  for (;;) {
    uint64_t type, size;
    RINOK7(rd_num(s, &type));
    if (type == kEnd) break;
    RINOK7(rd_num(s, &size));
    if (size > s.n) return SZ_ERROR_ARCHIVE;
    if (type > 0x7FFFFFFFull) {
      RINOK7(skip_size(s, size));
      continue;
    }
    switch (type) {
      case kName: {
        RINOK7(rd_switch(s));
        const size_t ns = size_t(size) - 1;
        if (ns & 1) return SZ_ERROR_ARCHIVE;
        if (ns > s.n) return SZ_ERROR_ARCHIVE;
        x.names.assign(s.p, s.p + ns);
        RINOK7(read_file_names(s.p, ns >> 1, nf, &x.name_offsets));
        RINOK7(skip_size(s, ns));
        break;
      }
      case kEmptyStream:
        RINOK7(bool_vec(s, nf, &empty_stream));
        n_empty = 0;
        for (Byte b : empty_stream) n_empty += b;
        break;
      case kEmptyFile:
        RINOK7(bool_vec(s, n_empty, &empty_file));
        break;
      case kWinAttributes:
      case kMTime: {
        RINOK7(bool_vec2(s, nf, &defined));
        RINOK7(rd_switch(s));
        for (uint32_t i = 0; i < nf; ++i)
          if (defined[i]) {
            uint32_t v;
            RINOK7(rd_u32(s, &v));
            if (type == kMTime) RINOK7(rd_u32(s, &v));
          }
        break;
      }
      default:
        RINOK7(skip_size(s, size));
    }
  }
  uint32_t ei = 0, si = 0;
  for (uint32_t i = 0; i < nf; ++i) {
    FileItem& f = x.files[i];
    f.has_stream = empty_stream.empty() ? true : empty_stream[i] == 0;
    if (f.has_stream) {
      // the reference indexes its substream arrays here unchecked
      if (!have_ss || si >= ss.n) return SZ_ERROR_ARCHIVE;
      f.is_dir = false;
      f.size = ss.sizes[si];
      f.crc = ss.digests[si];
      f.crc_defined = ss.defined[si] != 0;
      ++si;
    } else {
      f.is_dir = empty_file.empty() ? true : (ei < empty_file.size() ? empty_file[ei] == 0 : true);
      ++ei;
      f.size = 0;
      f.crc = 0;
      f.crc_defined = false;
    }
  }
  return fill(x);
}

// One coder of a folder that produces bytes from a pack stream (Copy / LZMA /
// LZMA2): its input range in the archive, its output size and where it goes.
struct Unit {
  uint64_t pack_off = 0, pack_size = 0, avail = 0, unpack = 0, dst_off = 0;
  uint64_t method = 0;
  std::vector<Byte> props;
  bool tmp = false;    // output in the BCJ2 temp buffer, not the folder output
  SRes pre = SZ_OK;    // checks before decoding (props, Copy sizes, truncation)
  SRes res = SZ_OK;    // after decoding
};

// One folder's decode job: SzFolder_Decode2 (7zDec.c:335-471).  units[0] is the
// main coder of the 1- and 2-coder shapes; a BCJ2 folder has three units in
// coder order 0, 1, 2 (JMP stream, CALL stream, main stream) and its range-
// coder stream (pack stream 1) read raw from the archive.
struct Job {
  uint64_t pack_off = 0, pack_size = 0, unpack = 0, dst_off = 0;
  std::vector<Unit> units;
  bool x86 = false;
  bool arm = false;
  bool bcj2 = false;
  uint64_t rc_off = 0, rc_size = 0, rc_avail = 0;
  SRes res = SZ_OK;
};

// A coder's checks before it decodes: SzDecodeCopy / SzDecodeLzma /
// SzDecodeLzma2 (7zDec.c:127-241) as far as they fail without decoding.
static void unit_checks(Unit& u) {
  u.pre = SZ_OK;
  if (u.method == kCopy) {
    if (u.pack_size != u.unpack) u.pre = SZ_ERROR_DATA;
    else if (u.avail < u.pack_size) u.pre = SZ_ERROR_INPUT_EOF;
  } else if (u.method == kLzma) {
    // LzmaProps_Decode (LzmaDec.c:898-922)
    if (u.props.size() < 5 || u.props[0] >= 9 * 5 * 5) u.pre = SZ_ERROR_UNSUPPORTED;
  } else if (u.method == kPpmd) {
    // SzDecodePpmd (7zDec.c:80-90)
    if (u.props.size() != LZMA_GPU_PPMD7_PROPS_SIZE) {
      u.pre = SZ_ERROR_UNSUPPORTED;
    } else {
      const uint32_t order = u.props[0];
      const uint32_t mem = u.props[1] | (u.props[2] << 8) | (u.props[3] << 16) |
                           (uint32_t(u.props[4]) << 24);
      if (order < 2 || order > 64 || mem < (1u << 11) || mem > 0xFFFFFFFFu - 36u)
        u.pre = SZ_ERROR_UNSUPPORTED;
    }
  } else {
    // SzDecodeLzma2 (7zDec.c:181-183) + Lzma2Dec_GetOldProps (Lzma2Dec.c:69)
    if (u.props.size() != 1) u.pre = SZ_ERROR_DATA;
    else if (u.props[0] > 40) u.pre = SZ_ERROR_UNSUPPORTED;
  }
}

// CheckSupportedFolder (7zDec.c:269-322) and the job of each folder shape.
Job make_job(const Archive& x, const Ar& a, uint32_t fi, uint64_t start, const Byte*, size_t size) {
  Job j;
  const Folder& f = a.folders[fi];
  j.unpack = f.unpack_size();
  // PPMd (LZMA_GPU_7Z_PPMD) is a main method of the 1- and 2-coder shapes only:
  // inside a BCJ2 folder it stays unsupported
  auto main_ok = [](const Coder& c, bool ppmd = false) {
    return c.nin == 1 && c.nout == 1 && c.method <= 0xFFFFFFFFull &&
           (c.method == kCopy || c.method == kLzma || c.method == kLzma2 ||
            (ppmd && c.method == kPpmd));
  };
  const size_t nc = f.coders.size();
  j.res = SZ_ERROR_UNSUPPORTED;
  if (nc < 1 || nc > 4) return j;
  if (!main_ok(f.coders[0], (x.flags & LZMA_GPU_7Z_PPMD) != 0 && nc <= 2)) return j;
  const uint32_t ps = x.folder_start_pack.empty() ? 0 : x.folder_start_pack[fi];
  auto pack_size = [&](uint32_t k) {
    return ps + k < a.pack_sizes.size() ? a.pack_sizes[ps + k] : uint64_t(0);
  };
  // pack stream k of the folder starts behind streams 0..k-1 (GetSum, 7zDec.c:325)
  auto pack_at = [&](uint32_t k) {
    uint64_t o = start;
    for (uint32_t i = 0; i < k; ++i) o += pack_size(i);
    return o;
  };
  auto avail = [&](uint64_t off, uint64_t n) {
    return off >= size ? uint64_t(0) : std::min<uint64_t>(n, size - off);
  };
  auto unit = [&](const Coder& c, uint32_t si, uint64_t unpack) {
    Unit u;
    u.method = c.method;
    u.props = c.props;
    u.pack_size = pack_size(si);
    u.pack_off = pack_at(si);
    u.avail = avail(u.pack_off, u.pack_size);
    u.unpack = unpack;
    unit_checks(u);
    return u;
  };
  if (nc == 1) {
    if (f.pack_streams.size() != 1 || f.pack_streams[0] != 0 || !f.bind.empty()) return j;
  } else if (nc == 2) {
    const Coder& c = f.coders[1];
    if (c.method > 0xFFFFFFFFull || c.nin != 1 || c.nout != 1 || f.pack_streams.size() != 1 ||
        f.pack_streams[0] != 0 || f.bind.size() != 1 || f.bind[0].in != 1 || f.bind[0].out != 0)
      return j;
    if (c.method == kBcj)
      j.x86 = true;
    else if (c.method == kArm)
      j.arm = true;  // CASE_BRA_CONV(ARM), 7zDec.c:449
    else
      return j;
  } else if (nc == 4) {
    // IS_BCJ2 and the only bind layout the reference accepts (7zDec.c:303-319)
    const Coder& b = f.coders[3];
    if (!main_ok(f.coders[1]) || !main_ok(f.coders[2]) || b.method != kBcj2 || b.nin != 4 ||
        b.nout != 1)
      return j;
    static const uint32_t kPs[4] = {2, 6, 1, 0};
    static const uint32_t kBin[3] = {5, 4, 3}, kBout[3] = {0, 1, 2};
    if (f.pack_streams.size() != 4 || f.bind.size() != 3) return j;
    for (int k = 0; k < 4; ++k)
      if (f.pack_streams[k] != kPs[k]) return j;
    for (int k = 0; k < 3; ++k)
      if (f.bind[k].in != kBin[k] || f.bind[k].out != kBout[k]) return j;
    if (f.unpack_sizes.size() < 4) return j;
    j.bcj2 = true;
    // coder ci reads pack stream {3, 2, 0}[ci] (7zDec.c:356-359)
    static const uint32_t kSi[3] = {3, 2, 0};
    for (uint32_t ci = 0; ci < 3; ++ci) {
      j.units.push_back(unit(f.coders[ci], kSi[ci], f.unpack_sizes[ci]));
      j.units.back().tmp = ci < 2;
    }
    j.rc_off = pack_at(1);
    j.rc_size = pack_size(1);
    j.rc_avail = avail(j.rc_off, j.rc_size);
    j.pack_off = j.units[2].pack_off;  // the main stream's coder
    j.pack_size = j.units[2].pack_size;
    // coder 0 decodes first: what fails it before decoding fails the folder
    // (later coders' checks only count once the ones before them have decoded)
    j.res = j.units[0].pre;
    return j;
  } else {
    return j;
  }
  j.units.push_back(unit(f.coders[0], 0, j.unpack));
  j.pack_off = j.units[0].pack_off;
  j.pack_size = j.units[0].pack_size;
  j.res = j.units[0].pre;
  return j;
}

// Bytes of BCJ2 temp output (the CALL and JMP streams) a job list needs.
uint64_t bcj2_temp_bytes(const std::vector<Job>& jobs) {
  uint64_t t = 0;
  for (const Job& j : jobs)
    if (j.bcj2)
      for (const Unit& u : j.units)
        if (u.tmp) t += u.unpack;
  return t;
}

// SzDecodeLzma / SzDecodeLzma2 acceptance (7zDec.c:161-168, 209-216): the
// whole output, the whole pack stream, a finished status
static SRes accept(const Unit& u, const LzmaGpuResult& q) {
  // SzDecodeLzma and SzDecodeLzma2 never return SZ_ERROR_INPUT_EOF: input that
  // runs out ends as SZ_ERROR_DATA (7zDec.c:157-163, 207-212).  The batch
  // decoder says INPUT_EOF for an LZMA stream of fewer than the five bytes a
  // range coder starts with; the reference feeds what there is, gets nothing
  // decoded from an empty second look and says DATA.  Mapped for both kinds.
  if (q.res == SZ_ERROR_INPUT_EOF) return SZ_ERROR_DATA;
  if (q.res != SZ_OK) return q.res;
  const bool status_ok = u.method == kLzma ? (q.status == LZMA_STATUS_FINISHED_WITH_MARK ||
                                              q.status == LZMA_STATUS_MAYBE_FINISHED_WITHOUT_MARK)
                                           : q.status == LZMA_STATUS_FINISHED_WITH_MARK;
  if (q.dest_len != u.unpack || q.src_len != u.avail || u.avail != u.pack_size || !status_ok)
    return SZ_ERROR_DATA;
  return SZ_OK;
}

// The PPMd kernel's launcher lives in ppmd7_kernels.hip; a build of this file
// without it (the container fuzzer's host objects, tests/fuzz/) still links:
// the reference is weak, and a PPMd folder without the kernel is an error.
extern "C" __attribute__((weak)) int ppmd7gpu_launch(const Ppmd7GpuStreamDesc* d_descs, uint32_t n,
                                                     const uint8_t* d_src, uint8_t* d_dst,
                                                     uint8_t* d_ws, Ppmd7GpuResult* d_results,
                                                     hipStream_t stream);

// The PPMd units of a list as one PPMd7 batch launch on a stream of its own,
// beside the LZMA batch: start() queues it, finish() waits and sets each
// unit's res to SzDecodePpmd's.
struct PpmdBatch {
  std::vector<Unit*> which;
  DevArr<Byte> d_ws;
  DevArr<Ppmd7GpuStreamDesc> d_desc;
  DevArr<Ppmd7GpuResult> d_res;
  hipStream_t stream = nullptr;
  ~PpmdBatch() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  SRes start(std::vector<Unit*>& us, const Byte* d_arc, Byte* dst) {
    std::vector<Unit*> found;
    for (Unit* u : us)
      if (u->method == kPpmd) found.push_back(u);
    const size_t n = found.size();
    if (n == 0) return SZ_OK;
    std::vector<Ppmd7GpuStreamDesc> descs(n);
    for (size_t k = 0; k < n; ++k) {
      const Unit& u = *found[k];
      Ppmd7GpuStreamDesc& d = descs[k];
      d.src_off = u.pack_off;
      d.src_len = u.avail;
      d.dst_off = u.dst_off;
      d.dst_len = u.unpack;
      d.order = u.props[0];
      d.mem_size = u.props[1] | (u.props[2] << 8) | (u.props[3] << 16) | (uint32_t(u.props[4]) << 24);
    }
    // one launch, longest first (no limit: the plan cannot fail)
    LaunchPlan p;
    launch_plan(n, [&](uint32_t i) { return descs[i].dst_len; },
                [&](uint32_t i) { return ppmd7_slice_bytes(descs[i].mem_size); }, ~uint64_t(0), p);
    descs = in_launch_order(descs.data(), p);
    for (size_t k = 0; k < n; ++k) which.push_back(found[p.order[k]]);
    SRes r = alloc_all("7z", d_ws, size_t(p.ws_max), d_res, n);
    if (r != SZ_OK) return r;
    if (!hip_ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "7z PPMd stream"))
      return SZ_ERROR_FAIL;
    if ((r = upload(d_desc, descs, "7z")) != SZ_OK) return r;
    if (!ppmd7gpu_launch ||
        ppmd7gpu_launch(d_desc.p, uint32_t(n), d_arc, dst, d_ws.p, d_res.p, stream) != 0) {
      set_error("7z: PPMd7 batch kernel launch failed");
      return SZ_ERROR_FAIL;
    }
    return SZ_OK;
  }
  SRes finish() {
    const size_t n = which.size();
    if (n == 0) return SZ_OK;
    std::vector<Ppmd7GpuResult> res(n);
    if (!hip_ok(hipStreamSynchronize(stream), "7z PPMd decode") || !download(res, d_res.p, "7z D2H"))
      return SZ_ERROR_FAIL;
    for (size_t k = 0; k < n; ++k) {
      const Unit& u = *which[k];
      // a pack stream cut short by the archive's end cannot have been consumed whole
      which[k]->res = res[k].res != SZ_OK ? res[k].res
                      : u.avail != u.pack_size ? SZ_ERROR_DATA : SZ_OK;
    }
    return SZ_OK;
  }
};

// Decodes a list of units whose outputs go to `dst` (device) in one batch
// (PPMd units: PpmdBatch).
static SRes decode_units(std::vector<Unit*>& us, const Byte* d_arc, Byte* dst) {
  std::vector<LzmaGpuStreamDesc> descs;
  std::vector<Unit*> which;
  for (Unit* u : us) {
    if (u->method == kPpmd) continue;
    if (u->method == kCopy) {
      if (u->unpack && !hip_ok(hipMemcpyAsync(dst + u->dst_off, d_arc + u->pack_off, u->unpack,
                                              hipMemcpyDeviceToDevice, nullptr),
                               "7z copy coder"))
        return SZ_ERROR_FAIL;
      u->res = SZ_OK;
      continue;
    }
    LzmaGpuStreamDesc d;
    memset(&d, 0, sizeof d);
    d.src_off = u->pack_off;
    d.src_len = u->avail;
    d.dst_off = u->dst_off;
    d.dst_cap = u->unpack;
    d.finish_mode = LZMA_FINISH_END;
    if (u->method == kLzma) {
      memcpy(d.props, u->props.data(), 5);
      d.props_size = 5;
      d.kind = LZMA_GPU_KIND_LZMA;
    } else {
      d.props[0] = u->props[0];
      d.props_size = 1;
      d.kind = LZMA_GPU_KIND_LZMA2;
    }
    descs.push_back(d);
    which.push_back(u);
  }
  const size_t n = descs.size();
  if (n == 0) return SZ_OK;
  std::vector<LzmaGpuResult> res(n);
  std::vector<uint32_t> order(n);
  LzmaGpuPlan plan;
  SRes r = LzmaGpu_PlanBatchEx(descs.data(), n, order.data(), &plan);
  if (r != SZ_OK) return r;
  DevArr<Byte> d_ws;
  DevArr<LzmaGpuStreamDesc> d_desc;
  DevArr<uint32_t> d_order;
  DevArr<LzmaGpuResult> d_res;
  if ((r = alloc_all("7z", d_ws, size_t(plan.workspace_bytes), d_res, n)) != SZ_OK ||
      (r = upload(d_desc, descs, "7z")) != SZ_OK || (r = upload(d_order, order, "7z")) != SZ_OK ||
      (r = LzmaGpu_DecodeBatchEx(&plan, d_desc.p, d_order.p, d_arc, dst, d_ws.p, d_res.p,
                                 nullptr)) != SZ_OK)
    return r;
  if (!hip_ok(hipDeviceSynchronize(), "7z decode") || !download(res, d_res.p, "7z D2H"))
    return SZ_ERROR_FAIL;
  for (size_t k = 0; k < n; ++k) which[k]->res = accept(*which[k], res[k]);
  return SZ_OK;
}

// Runs the folder jobs on the GPU from the archive already in d_arc, output
// at each job's dst_off in d_dst; sets each job's res to SzFolder_Decode's.
// d_dst holds bcj2_temp_bytes(jobs) more bytes behind the folder outputs
// (at dst_bytes): the BCJ2 folders' CALL and JMP streams.
SRes run_jobs(std::vector<Job>& jobs, const Byte* d_arc, Byte* d_dst, uint64_t dst_bytes) {
  std::vector<Unit*> units;
  std::vector<uint64_t> bcj_off, bcj_len, arm_off, arm_len;
  uint64_t tmp = dst_bytes;
  for (Job& j : jobs) {
    if (j.res != SZ_OK) continue;
    if (!j.bcj2) {
      Unit& u = j.units[0];
      u.dst_off = j.dst_off;
      units.push_back(&u);
      if (j.x86 && j.unpack) {
        bcj_off.push_back(j.dst_off);
        bcj_len.push_back(j.unpack);
      }
      if (j.arm && j.unpack) {
        arm_off.push_back(j.dst_off);
        arm_len.push_back(j.unpack);
      }
      continue;
    }
    // SzFolder_Decode2 stops at the first failing coder, in coder order; the
    // main stream coder (2) first checks that its output fits (7zDec.c:370)
    for (uint32_t ci = 0; ci < 3; ++ci) {
      Unit& u = j.units[ci];
      if (ci == 2 && u.unpack > j.unpack) break;
      if (u.pre != SZ_OK) break;
      if (u.tmp) {
        u.dst_off = tmp;
        tmp += u.unpack;
      } else {
        u.dst_off = j.dst_off + (j.unpack - u.unpack);  // the tail of the folder output
      }
      units.push_back(&u);
    }
  }
  {
    PpmdBatch ppmd;
    RINOK7(ppmd.start(units, d_arc, d_dst));
    const SRes lz = decode_units(units, d_arc, d_dst);
    RINOK7(ppmd.finish());  // also on an LZMA-side error: nothing stays queued
    RINOK7(lz);
  }
  // BCJ2 folders: the first failure in coder order, else the rc stream and
  // Bcj2_Decode (7zDec.c:423-441)
  std::vector<Bcj2GpuJob> b2;
  std::vector<Job*> b2_job;
  for (Job& j : jobs) {
    if (j.res != SZ_OK) continue;
    if (!j.bcj2) {
      j.res = j.units[0].res;
      continue;
    }
    SRes r = SZ_OK;
    for (uint32_t ci = 0; ci < 3 && r == SZ_OK; ++ci) {
      const Unit& u = j.units[ci];
      if (ci == 2 && u.unpack > j.unpack) r = SZ_ERROR_PARAM;
      else if (u.pre != SZ_OK) r = u.pre;
      else r = u.res;
    }
    if (r == SZ_OK && j.rc_avail < j.rc_size) r = SZ_ERROR_INPUT_EOF;  // SzDecodeCopy
    j.res = r;
    if (r != SZ_OK) continue;
    Bcj2GpuJob q;
    q.buf0 = d_dst + j.units[2].dst_off;
    q.size0 = j.units[2].unpack;
    q.buf1 = d_dst + j.units[1].dst_off;  // CALL stream: coder 1 (tempBuf[0])
    q.size1 = j.units[1].unpack;
    q.buf2 = d_dst + j.units[0].dst_off;  // JMP stream: coder 0 (tempBuf[1])
    q.size2 = j.units[0].unpack;
    q.buf3 = d_arc + j.rc_off;
    q.size3 = j.rc_size;
    q.out = d_dst + j.dst_off;
    q.out_size = j.unpack;
    b2.push_back(q);
    b2_job.push_back(&j);
  }
  if (!b2.empty()) {
    const size_t n = b2.size();
    DevArr<Bcj2GpuJob> d_jobs;
    DevArr<int32_t> d_res;
    std::vector<int32_t> res(n);
    RINOK7(upload(d_jobs, b2, "7z"));
    RINOK7(alloc_all("7z", d_res, n));
    RINOK7(Bcj2Gpu_Batch(d_jobs.p, n, d_res.p, nullptr));
    if (!hip_ok(hipDeviceSynchronize(), "7z BCJ2") || !download(res, d_res.p, "7z D2H"))
      return SZ_ERROR_FAIL;
    for (size_t k = 0; k < n; ++k) b2_job[k]->res = res[k];
  }
  // x86_Convert(outBuffer, outSize, 0, &state0, 0) per BCJ folder, then
  // ARM_Convert(outBuffer, outSize, 0, 0) per ARM folder
  FilterJob x86, arm;
  RINOK7(queue_filter("7z", x86, 4, d_dst, bcj_off, bcj_len, nullptr, 0));
  if (!hip_ok(hipDeviceSynchronize(), "7z BCJ")) return SZ_ERROR_FAIL;
  RINOK7(queue_filter("7z", arm, 7, d_dst, arm_off, arm_len, nullptr, 0));
  if (!arm_off.empty() && !hip_ok(hipDeviceSynchronize(), "7z ARM")) return SZ_ERROR_FAIL;
  return SZ_OK;
}

// Folder outputs tile one device buffer, BCJ2 temp streams behind them
// (sz_extract, the packed-header decode below): every size a folder states
// goes into one running sum, and a sum that wraps or reaches 2^63 ends the
// open with SZ_ERROR_MEM -- what SzArEx_Extract returns when a folder's size
// cannot be allocated (7zIn.c:1354-1369).  7z numbers are full 64-bit, so two
// folders are enough to wrap a plain sum.
SRes sizes_checked(const Ar& a) {
  uint64_t sum = 0;
  for (const Folder& f : a.folders)
    for (const uint64_t v : f.unpack_sizes) {
      if (v >= (uint64_t(1) << 63) - sum) return SZ_ERROR_MEM;
      sum += v;
    }
  return SZ_OK;
}

// SzArEx_Open2 (7zIn.c:1214-1312)
SRes open_archive(const Byte* arc, size_t size, Archive& x) {
  if (size < kStartHeader) return SZ_ERROR_NO_ARCHIVE;
  static const Byte sig[6] = {'7', 'z', 0xBC, 0xAF, 0x27, 0x1C};
  if (memcmp(arc, sig, 6) != 0) return SZ_ERROR_NO_ARCHIVE;
  if (arc[6] != 0) return SZ_ERROR_UNSUPPORTED;
  uint64_t off = 0, hsize = 0;
  uint32_t hcrc = 0, scrc = 0;
  for (int i = 7; i >= 0; --i) off = (off << 8) | arc[12 + i];
  for (int i = 7; i >= 0; --i) hsize = (hsize << 8) | arc[20 + i];
  for (int i = 3; i >= 0; --i) hcrc = (hcrc << 8) | arc[28 + i];
  for (int i = 3; i >= 0; --i) scrc = (scrc << 8) | arc[8 + i];
  if (crc32_host(arc + 12, 20) != scrc) return SZ_ERROR_CRC;
  if (hsize == 0) return SZ_OK;
  if (off > off + hsize || off > off + hsize + kStartHeader) return SZ_ERROR_NO_ARCHIVE;
  if (uint64_t(size) < off + kStartHeader + hsize || uint64_t(size) < off + kStartHeader)
    return SZ_ERROR_INPUT_EOF;
  const Byte* h = arc + kStartHeader + off;
  if (crc32_host(h, size_t(hsize)) != hcrc) return SZ_ERROR_ARCHIVE;
  Sd s{h, size_t(hsize)};
  uint64_t t;
  RINOK7(rd_num(s, &t));
  std::vector<Byte> unpacked;
  if (t == kEncodedHeader) {
    // SzReadAndDecodePackedStreams2 (7zIn.c:1147-1189): one folder, on the GPU
    Archive hx;
    SubStreams ss;
    bool have_ss = false;
    uint64_t start = 0;
    RINOK7(read_streams_info(s, &start, hx.db, ss, &have_ss));
    start += kStartHeader;
    if (hx.db.folders.size() != 1) return SZ_ERROR_ARCHIVE;
    // no PackInfo, or fewer sizes than the folder has pack streams: the
    // reference reads PackSizes unchecked (7zIn.c:1181, 7zDec.c:385-386)
    if (hx.db.folders[0].pack_streams.size() > hx.db.pack_sizes.size()) return SZ_ERROR_ARCHIVE;
    RINOK7(sizes_checked(hx.db));
    hx.folder_start_pack.assign(1, 0);
    hx.flags = x.flags;
    std::vector<Job> jobs(1, make_job(hx, hx.db, 0, start, arc, size));
    const Folder& f = hx.db.folders[0];
    if (jobs[0].res != SZ_OK) return jobs[0].res;
    unpacked.resize(size_t(f.unpack_size()));
    if (!ensure_device()) return SZ_ERROR_FAIL;
    // only the header's pack stream goes to the device (a BCJ2-packed header:
    // the archive)
    const bool one = !jobs[0].bcj2;
    const uint64_t at = one ? jobs[0].units[0].pack_off : 0;
    const uint64_t nbytes = one ? jobs[0].units[0].avail : uint64_t(size);
    if (one) jobs[0].units[0].pack_off = 0;
    DevArr<Byte> d_arc, d_out;
    RINOK7(alloc_all("7z", d_arc, size_t(nbytes), d_out,
                     unpacked.size() + size_t(bcj2_temp_bytes(jobs))));
    if (nbytes && !hip_ok(hipMemcpy(d_arc.p, arc + at, size_t(nbytes), hipMemcpyHostToDevice),
                          "7z H2D"))
      return SZ_ERROR_FAIL;
    RINOK7(run_jobs(jobs, d_arc.p, d_out.p, unpacked.size()));
    if (jobs[0].res != SZ_OK) return jobs[0].res;
    if (!unpacked.empty() &&
        !hip_ok(hipMemcpy(unpacked.data(), d_out.p, unpacked.size(), hipMemcpyDeviceToHost),
                "7z D2H"))
      return SZ_ERROR_FAIL;
    if (f.crc_defined && crc32_host(unpacked.data(), unpacked.size()) != f.crc)
      return SZ_ERROR_CRC;
    s = Sd{unpacked.data(), unpacked.size()};
    RINOK7(rd_num(s, &t));
  }
  if (t != kHeader) return SZ_ERROR_UNSUPPORTED;
  return read_header(x, s);
}

SRes open_checked(const Byte* arc, size_t size, Archive& x, unsigned flags) {
  x.flags = flags;
  SRes r = open_archive(arc, size, x);
  if (r == SZ_OK) r = sizes_checked(x.db);  // before any caller lays folders out
  if (r != SZ_OK) x = Archive();
  return r;
}

}  // namespace

static SRes sz_open(const Byte* archive, size_t size, LzmaGpu7zFolder* folders, size_t folder_cap,
                    size_t* n_folders, LzmaGpu7zFile* files, size_t file_cap, size_t* n_files,
                    UInt16* names, size_t names_cap, size_t* names_len, UInt64* unpack_total,
                    unsigned flags) {
  Archive x;
  const SRes r = open_checked(archive, size, x, flags);
  if (n_folders) *n_folders = x.db.folders.size();
  if (n_files) *n_files = x.files.size();
  if (names_len) *names_len = x.names.size() / 2;
  uint64_t total = 0;
  std::vector<uint64_t> fdst(x.db.folders.size(), 0);
  for (size_t i = 0; i < x.db.folders.size(); ++i) {
    fdst[i] = total;
    total += x.db.folders[i].unpack_size();
  }
  if (unpack_total) *unpack_total = total;
  if (r != SZ_OK) return r;
  for (size_t i = 0; i < x.db.folders.size() && folders && i < folder_cap; ++i) {
    const Folder& f = x.db.folders[i];
    const Job j = make_job(x, x.db, uint32_t(i),
                           x.db.data_pos + (x.folder_start_pack[i] < x.pack_start.size()
                                                ? x.pack_start[x.folder_start_pack[i]]
                                                : 0),
                           archive, size);
    LzmaGpu7zFolder& o = folders[i];
    memset(&o, 0, sizeof o);
    o.pack_off = j.pack_off;
    o.pack_size = j.pack_size;
    o.unpack_size = f.unpack_size();
    o.dst_off = fdst[i];
    o.method = f.coders.empty() ? 0 : f.coders[0].method;
    o.x86 = j.x86 ? 1 : 0;
    o.supported = uint32_t(j.res);
    o.crc_defined = f.crc_defined ? 1 : 0;
    o.crc = f.crc;
    o.first_file = x.folder_start_file[i];
    o.num_files = f.num_unpack_streams;
    o.num_coders = uint32_t(f.coders.size());
    if (!f.coders.empty()) {
      const std::vector<Byte>& p = f.coders[0].props;
      o.props_size = uint32_t(p.size());
      if (!p.empty()) memcpy(o.props, p.data(), std::min<size_t>(p.size(), sizeof o.props));
    }
  }
  for (size_t i = 0; i < x.files.size() && files && i < file_cap; ++i) {
    const FileItem& f = x.files[i];
    LzmaGpu7zFile& o = files[i];
    memset(&o, 0, sizeof o);
    o.size = f.size;
    o.folder = x.file_folder[i];
    if (o.folder != kNoFolder) {
      uint64_t off = fdst[o.folder];
      for (uint32_t k = x.folder_start_file[o.folder]; k < i; ++k) off += uint32_t(x.files[k].size);
      o.dst_off = off;
    }
    o.crc = f.crc;
    o.crc_defined = f.crc_defined ? 1 : 0;
    o.has_stream = f.has_stream ? 1 : 0;
    o.is_dir = f.is_dir ? 1 : 0;
    if (!x.name_offsets.empty()) {
      o.name_off = uint32_t(x.name_offsets[i]);
      o.name_len = uint32_t(x.name_offsets[i + 1] - x.name_offsets[i]);
    }
  }
  if (names)
    for (size_t i = 0; i < x.names.size() / 2 && i < names_cap; ++i)
      names[i] = UInt16(x.names[2 * i] | (x.names[2 * i + 1] << 8));
  return SZ_OK;
}

// A file's range inside its folder's output.  A substream size is the folder's
// size minus the sizes before it, which wraps where those exceed it (line
// 7zIn.c:792 wraps the same way), so off + len is not formed.
static bool file_fits(uint64_t off, uint64_t len, uint64_t unpack) {
  return len <= unpack && off <= unpack - len;
}

static SRes sz_extract(Byte* dest, SizeT* destLen, const Byte* archive, size_t size,
                       SRes* file_res, size_t file_cap, unsigned flags) {
  const SizeT cap = *destLen;
  *destLen = 0;
  Archive x;
  SRes r = open_checked(archive, size, x, flags);
  if (r != SZ_OK) return r;
  const Ar& a = x.db;
  const size_t nf = a.folders.size(), nfiles = x.files.size();
  std::vector<Job> jobs(nf);
  uint64_t total = 0;
  for (size_t i = 0; i < nf; ++i) {
    const uint64_t start = a.data_pos + (x.folder_start_pack[i] < x.pack_start.size()
                                             ? x.pack_start[x.folder_start_pack[i]]
                                             : 0);
    jobs[i] = make_job(x, a, uint32_t(i), start, archive, size);
    jobs[i].dst_off = total;
    total += jobs[i].unpack;
  }
  if (total > cap) return SZ_ERROR_OUTPUT_EOF;
  // file ranges inside their folder's output (SzArEx_Extract's offset walk)
  std::vector<uint64_t> foff(nfiles, 0);
  std::vector<SRes> fres(nfiles, SZ_OK);
  for (size_t i = 0; i < nfiles; ++i) {
    const uint32_t fo = x.file_folder[i];
    if (fo == kNoFolder) continue;
    uint64_t off = 0;
    // SzArEx_Extract sums (UInt32)Files[k].Size (7zIn.c:1392)
    for (uint32_t k = x.folder_start_file[fo]; k < i; ++k) off += uint32_t(x.files[k].size);
    foff[i] = off;
  }
  if (nf) {
    if (!ensure_device()) return SZ_ERROR_FAIL;
    DevArr<Byte> d_arc, d_dst;
    RINOK7(alloc_all("7z", d_arc, size, d_dst, size_t(total + bcj2_temp_bytes(jobs))));
    if (!hip_ok(hipMemcpy(d_arc.p, archive, size, hipMemcpyHostToDevice), "7z H2D"))
      return SZ_ERROR_FAIL;
    RINOK7(run_jobs(jobs, d_arc.p, d_dst.p, total));
    // CRC-32 of every decoded folder with a CRC and of every file range
    std::vector<uint64_t> off, len;
    std::vector<int64_t> tag;  // >= 0: folder, < 0: ~file
    for (size_t i = 0; i < nf; ++i)
      if (jobs[i].res == SZ_OK && a.folders[i].crc_defined) {
        off.push_back(jobs[i].dst_off);
        len.push_back(jobs[i].unpack);
        tag.push_back(int64_t(i));
      }
    for (size_t i = 0; i < nfiles; ++i) {
      const uint32_t fo = x.file_folder[i];
      if (fo == kNoFolder || jobs[fo].res != SZ_OK || !x.files[i].crc_defined) continue;
      if (!file_fits(foff[i], x.files[i].size, jobs[fo].unpack)) continue;
      off.push_back(jobs[fo].dst_off + foff[i]);
      len.push_back(x.files[i].size);
      tag.push_back(~int64_t(i));
    }
    const size_t nc = off.size();
    std::vector<uint32_t> crc(nc);
    RangeChecks checks;
    RINOK7(checks.prepare("7z", 4, off, len));
    RINOK7(checks.launch(d_dst.p));
    if (nc && (!hip_ok(hipDeviceSynchronize(), "7z CRC") || !checks.fetch(crc.data(), "7z D2H")))
      return SZ_ERROR_FAIL;
    for (size_t k = 0; k < nc; ++k)
      if (tag[k] >= 0 && crc[k] != a.folders[size_t(tag[k])].crc) jobs[size_t(tag[k])].res = SZ_ERROR_CRC;
    for (size_t i = 0; i < nfiles; ++i) {
      const uint32_t fo = x.file_folder[i];
      if (fo == kNoFolder) continue;
      if (jobs[fo].res != SZ_OK) {
        fres[i] = jobs[fo].res;
      } else if (!file_fits(foff[i], x.files[i].size, jobs[fo].unpack)) {
        fres[i] = SZ_ERROR_FAIL;
      }
    }
    for (size_t k = 0; k < nc; ++k)
      if (tag[k] < 0) {
        const size_t i = size_t(~tag[k]);
        if (fres[i] == SZ_OK && crc[k] != x.files[i].crc) fres[i] = SZ_ERROR_CRC;
      }
    if (total && !hip_ok(hipMemcpy(dest, d_dst.p, total, hipMemcpyDeviceToHost), "7z D2H"))
      return SZ_ERROR_FAIL;
  }
  SRes first = SZ_OK;
  for (size_t i = 0; i < nfiles; ++i) {
    if (file_res && i < file_cap) file_res[i] = fres[i];
    if (first == SZ_OK) first = fres[i];
  }
  *destLen = SizeT(total);
  return first;
}

// C ABI: no exception crosses it.  Host allocation failures (a header that
// asks for more than the host has) return SZ_ERROR_MEM, as the reference's
// MY_ALLOC / Buf_Create do (7zIn.c:496, 659, 1215).
SRes LzmaGpu_7zOpenEx(const Byte* archive, size_t size, LzmaGpu7zFolder* folders,
                      size_t folder_cap, size_t* n_folders, LzmaGpu7zFile* files, size_t file_cap,
                      size_t* n_files, UInt16* names, size_t names_cap, size_t* names_len,
                      UInt64* unpack_total, unsigned flags) {
  if (flags & ~LZMA_GPU_7Z_KNOWN_FLAGS) return SZ_ERROR_PARAM;
  return guarded("7z: host allocation failed", [&]() {
    return sz_open(archive, size, folders, folder_cap, n_folders, files, file_cap, n_files, names,
                   names_cap, names_len, unpack_total, flags);
  });
}

SRes LzmaGpu_7zExtractEx(Byte* dest, SizeT* destLen, const Byte* archive, size_t size,
                         SRes* file_res, size_t file_cap, unsigned flags) {
  if (flags & ~LZMA_GPU_7Z_KNOWN_FLAGS) return SZ_ERROR_PARAM;
  return guarded("7z: host allocation failed", [&]() {
    return sz_extract(dest, destLen, archive, size, file_res, file_cap, flags);
  });
}

SRes LzmaGpu_7zOpen(const Byte* archive, size_t size, LzmaGpu7zFolder* folders, size_t folder_cap,
                    size_t* n_folders, LzmaGpu7zFile* files, size_t file_cap, size_t* n_files,
                    UInt16* names, size_t names_cap, size_t* names_len, UInt64* unpack_total) {
  return LzmaGpu_7zOpenEx(archive, size, folders, folder_cap, n_folders, files, file_cap, n_files,
                          names, names_cap, names_len, unpack_total, 0);
}

SRes LzmaGpu_7zExtract(Byte* dest, SizeT* destLen, const Byte* archive, size_t size,
                       SRes* file_res, size_t file_cap) {
  return LzmaGpu_7zExtractEx(dest, destLen, archive, size, file_res, file_cap, 0);
}
