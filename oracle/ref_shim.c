/*
 * ref_shim.c -- TEST INFRASTRUCTURE ONLY.
 *
 * ctypes wrappers around the reference's CONTAINER and filter code (xz and 7z
 * readers, x86 BCJ, CRC-64; the Bra / Delta / Bcj2 / CRC-32 functions are
 * called directly), compiled in place from /root/reference by
 * oracle/Makefile.ref into oracle/_ref/libref.so.  That library carries the
 * only stand-ins of the reference build, confined to it: 7zStream.c's
 * Windows-only TRUE constant (-DTRUE=1) and 7zFile.c's two Windows file
 * openers left to lazy binding (tests/native.py loads it RTLD_LAZY); neither
 * is on any path these wrappers drive.  The LZMA pin is oracle/_ref/
 * libref_lzma.so (ref_lzma_shim.c), built without them.
 *
 * Nothing in the product (lzma-sdk-zliblike_amd/) links or loads this.
 */
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "Alloc.h"
#include "LzmaDec.h"

/* the largest request the reference made since the last reset: the hand-made
 * 7z cases must not hang on whether a huge malloc succeeds (ref_shim_max_alloc) */
static size_t g_shim_max_alloc = 0;
static void *shim_alloc(void *p, size_t n) {
  (void)p;
  if (n > g_shim_max_alloc) g_shim_max_alloc = n;
  return malloc(n ? n : 1);
}
unsigned long long ref_shim_max_alloc(int reset) {
  unsigned long long m = g_shim_max_alloc;
  if (reset) g_shim_max_alloc = 0;
  return m;
}
static void shim_free(void *p, void *a) { (void)p; free(a); }
static ISzAlloc g_shim_alloc = {shim_alloc, shim_free};

static int quiet_begin(void) {
  int saved, devnull;
  fflush(stdout);
  saved = dup(1);
  devnull = open("/dev/null", O_WRONLY);
  if (devnull >= 0) { dup2(devnull, 1); close(devnull); }
  return saved;
}

static void quiet_end(int saved) {
  fflush(stdout);
  if (saved >= 0) { dup2(saved, 1); close(saved); }
}

/*
 * xz: XzUnpacker_Code (XzDec.c:604-870) over a whole
 * in-memory file, FINISH_END, in one call with an output buffer of *dst_len
 * bytes.  *done = XzUnpacker_IsStreamWasFinished (XzDec.c:872).  The CRC
 * tables (CrcGenerateTable, Crc64GenerateTable) are built on first use.
 */
#include "7zCrc.h"
#include "Bra.h"
#include "Xz.h"
#include "XzCrc64.h"

static void xz_tables(void) {
  static int done = 0;
  if (!done) { CrcGenerateTable(); Crc64GenerateTable(); done = 1; }
}

int ref_xz_decode(unsigned char *dst, size_t *dst_len, const unsigned char *src,
                  size_t *src_len, int *status, int *done) {
  CXzUnpacker u;
  SizeT dl = *dst_len, sl = *src_len;
  ECoderStatus st = CODER_STATUS_NOT_SPECIFIED;
  SRes res;
  int saved;
  xz_tables();
  saved = quiet_begin();
  XzUnpacker_Create(&u, &g_shim_alloc);
  res = XzUnpacker_Code(&u, dst, &dl, src, &sl, LZMA_FINISH_END, &st);
  *done = XzUnpacker_IsStreamWasFinished(&u) ? 1 : 0;
  XzUnpacker_Free(&u);
  quiet_end(saved);
  *dst_len = dl;
  *src_len = sl;
  *status = (int)st;
  return res;
}

/* x86 BCJ (Bra86.c:11) over a buffer: returns the bytes processed, state in/out. */
size_t ref_x86_convert(unsigned char *data, size_t size, unsigned ip, unsigned *state,
                       int encoding) {
  UInt32 s = *state;
  SizeT r = x86_Convert(data, size, ip, &s, encoding);
  *state = s;
  return r;
}

/* Crc64Calc (XzCrc64.c:30) */
unsigned long long ref_crc64(const unsigned char *data, size_t size) {
  xz_tables();
  return Crc64Calc(data, size);
}

/*
 * 7z archives: SzArEx_Open over an in-memory archive
 * through LookToRead (non-lookahead, as 7zMain.c:326 sets it up), then
 * SzArEx_Extract (7zIn.c:1322) for every file with a fresh folder cache
 * (blockIndex reset after an error, so each file's result stands alone).
 * Files that extract OK are appended to out; file_res / file_size per file
 * (REF_7Z_OUTSIDE where the reference reports OK for a range outside its own
 * buffer); names = the raw UTF-16LE FileNames buffer.  Returns SzArEx_Open's
 * result.
 */
#include "7z.h"

#define REF_7Z_OUTSIDE (-1)

typedef struct {
  ISeekInStream s;
  const Byte *data;
  size_t size, pos;
} ShimMemSeek;

static SRes shim_seek_read(void *pp, void *buf, size_t *size) {
  ShimMemSeek *m = (ShimMemSeek *)pp;
  size_t n = m->size - m->pos;
  if (n > *size) n = *size;
  memcpy(buf, m->data + m->pos, n);
  m->pos += n;
  *size = n;
  return SZ_OK;
}

static SRes shim_seek_seek(void *pp, Int64 *pos, ESzSeek origin) {
  ShimMemSeek *m = (ShimMemSeek *)pp;
  Int64 base = origin == SZ_SEEK_SET ? 0 : (origin == SZ_SEEK_CUR ? (Int64)m->pos : (Int64)m->size);
  Int64 np = base + *pos;
  if (np < 0) return SZ_ERROR_READ;
  m->pos = (size_t)np > m->size ? m->size : (size_t)np;
  *pos = np;
  return SZ_OK;
}

int ref_7z_extract(const unsigned char *arc, size_t size, unsigned char *out, size_t cap,
                   size_t *out_len, int *file_res, unsigned long long *file_size,
                   unsigned *n_files, unsigned max_files, unsigned char *names,
                   size_t names_cap, size_t *names_len) {
  ShimMemSeek ms;
  CLookToRead look;
  CSzArEx db;
  SRes res;
  UInt32 i, block = 0xFFFFFFFF;
  Byte *buf = 0;
  size_t buf_size = 0, pos = 0;
  int saved;
  xz_tables();
  ms.s.Read = shim_seek_read;
  ms.s.Seek = shim_seek_seek;
  ms.data = arc;
  ms.size = size;
  ms.pos = 0;
  LookToRead_CreateVTable(&look, False);
  look.realStream = &ms.s;
  LookToRead_Init(&look);
  saved = quiet_begin();
  SzArEx_Init(&db);
  res = SzArEx_Open(&db, &look.s, &g_shim_alloc, &g_shim_alloc);
  *n_files = 0;
  *names_len = 0;
  if (res == SZ_OK) {
    *n_files = db.db.NumFiles;
    if (db.FileNames.data && db.FileNames.size <= names_cap) {
      memcpy(names, db.FileNames.data, db.FileNames.size);
      *names_len = db.FileNames.size;
    }
    for (i = 0; i < db.db.NumFiles && i < max_files; i++) {
      size_t offset = 0, got = 0;
      SRes r = SzArEx_Extract(&db, &look.s, i, &block, &buf, &buf_size, &offset, &got,
                              &g_shim_alloc, &g_shim_alloc);
      /* a substream size that wrapped (7zIn.c:792) can pass SzArEx_Extract's
         offset + size check (7zIn.c:1395, a sum that wraps back): the range it
         then reports lies outside its own buffer and is not read here */
      if (r == SZ_OK && (got > buf_size || offset > buf_size - got)) r = REF_7Z_OUTSIDE;
      file_res[i] = r;
      file_size[i] = db.db.Files[i].Size;
      if (r == SZ_OK && got != 0 && got <= cap - pos) {
        memcpy(out + pos, buf + offset, got);
        pos += got;
      }
      if (r != SZ_OK) block = 0xFFFFFFFF;
    }
  }
  free(buf);
  SzArEx_Free(&db, &g_shim_alloc);
  quiet_end(saved);
  *out_len = pos;
  return res;
}

/*
 * What SzArEx_Open made of the header (the structures SzArEx_Extract walks):
 * per folder five UInt64s {NumCoders, SzFolder_GetUnpackSize, UnpackCRCDefined,
 * UnpackCRC, NumUnpackStreams}, per file five UInt32s {HasStream, IsDir,
 * CrcDefined, Crc, FileIndexToFolderIndexMap}; a CRC that is not defined is
 * given as 0 (the reference leaves its value unset).  Counts are complete even
 * where the arrays are too small.  Returns SzArEx_Open's result.
 */
int ref_7z_info(const unsigned char *arc, size_t size, unsigned long long *folders,
                size_t folder_cap, unsigned *n_folders, unsigned *files, size_t file_cap,
                unsigned *n_files) {
  ShimMemSeek ms;
  CLookToRead look;
  CSzArEx db;
  SRes res;
  UInt32 i;
  int saved;
  xz_tables();
  ms.s.Read = shim_seek_read;
  ms.s.Seek = shim_seek_seek;
  ms.data = arc;
  ms.size = size;
  ms.pos = 0;
  LookToRead_CreateVTable(&look, False);
  look.realStream = &ms.s;
  LookToRead_Init(&look);
  saved = quiet_begin();
  SzArEx_Init(&db);
  res = SzArEx_Open(&db, &look.s, &g_shim_alloc, &g_shim_alloc);
  *n_folders = 0;
  *n_files = 0;
  if (res == SZ_OK) {
    *n_folders = db.db.NumFolders;
    *n_files = db.db.NumFiles;
    for (i = 0; i < db.db.NumFolders && i < folder_cap; i++) {
      CSzFolder *f = db.db.Folders + i;
      folders[5 * i] = f->NumCoders;
      folders[5 * i + 1] = SzFolder_GetUnpackSize(f);
      folders[5 * i + 2] = f->UnpackCRCDefined ? 1 : 0;
      folders[5 * i + 3] = f->UnpackCRCDefined ? f->UnpackCRC : 0;
      folders[5 * i + 4] = f->NumUnpackStreams;
    }
    for (i = 0; i < db.db.NumFiles && i < file_cap; i++) {
      const CSzFileItem *f = db.db.Files + i;
      files[5 * i] = f->HasStream ? 1 : 0;
      files[5 * i + 1] = f->IsDir ? 1 : 0;
      files[5 * i + 2] = f->CrcDefined ? 1 : 0;
      files[5 * i + 3] = f->CrcDefined ? f->Crc : 0;
      files[5 * i + 4] = db.FileIndexToFolderIndexMap ? db.FileIndexToFolderIndexMap[i] : 0xFFFFFFFF;
    }
  }
  SzArEx_Free(&db, &g_shim_alloc);
  quiet_end(saved);
  return res;
}

/*
 * xz backward index (Xzs_ReadBackward, XzIn.c:274-306) over an in-memory file
 * through the seek stream above behind a CLookToRead.  Streams come out of the
 * reference last first; here everything is returned in file order:
 * stream_flags[s], and per block {stream, totalSize, unpackSize} as three
 * UInt64s in blocks[].  *unpack_total = Xzs_GetUnpackSize, XZ_SIZE_OVERFLOW
 * passed through.  Counts are complete even where the arrays are too small.
 */
int ref_xz_index(const unsigned char *file, size_t size, unsigned *n_streams,
                 unsigned short *stream_flags, size_t stream_cap, unsigned long long *blocks,
                 size_t block_cap, size_t *n_blocks, unsigned long long *unpack_total) {
  ShimMemSeek ms;
  CLookToRead look;
  CXzs xzs;
  Int64 start = 0;
  SRes res;
  size_t k, i, nb = 0;
  xz_tables();
  ms.s.Read = shim_seek_read;
  ms.s.Seek = shim_seek_seek;
  ms.data = file;
  ms.size = size;
  ms.pos = 0;
  LookToRead_CreateVTable(&look, False);
  look.realStream = &ms.s;
  LookToRead_Init(&look);
  Xzs_Construct(&xzs);
  res = Xzs_ReadBackward(&xzs, &look.s, &start, 0, &g_shim_alloc);
  *n_streams = 0;
  *n_blocks = 0;
  *unpack_total = 0;
  if (res == SZ_OK) {
    *n_streams = (unsigned)xzs.num;
    *unpack_total = Xzs_GetUnpackSize(&xzs);
    for (k = 0; k < xzs.num; k++) {
      const CXzStream *st = &xzs.streams[xzs.num - 1 - k];
      if (k < stream_cap) stream_flags[k] = st->flags;
      for (i = 0; i < st->numBlocks; i++, nb++)
        if (nb < block_cap) {
          blocks[3 * nb] = k;
          blocks[3 * nb + 1] = st->blocks[i].totalSize;
          blocks[3 * nb + 2] = st->blocks[i].unpackSize;
        }
    }
    *n_blocks = nb;
  }
  Xzs_Free(&xzs, &g_shim_alloc);
  return res;
}
