// range_capi.hip -- the C ABI of the byte-range primitives (include/lzma_gpu.h):
// the checks (CRC-32, CRC-64, SHA-256) and the in-place filters (x86 BCJ, the
// five RISC converters, delta, BCJ2 decode), each as a batch over device ranges
// and as the reference's drop-in over a host buffer (7zCrc.h, XzCrc64.h,
// Sha256.h, Bra.h, Delta.h, Bcj2.h).  The xz reader, the 7z reader and the 7z
// writer call the batch forms; the kernels are crc_kernels.hip,
// sha256_kernels.hip and filter_kernels.hip.
//
// A drop-in has no error channel: without a device, or when a device call
// fails, it returns 0 or leaves the data as it was, with the reason in
// LzmaGpu_LastError.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "crc_device.h"
#include "host_batch.h"
#include "lzma_gpu_internal.h"

using namespace lzgpu_host;

// ------------------------------------------------------------------ CRC-32, CRC-64

namespace {

// The chunk slots of n ranges, range i of len(i) bytes: chunk_base[i] = its
// first slot, chunk_range[slot] = its range (either may be null); returns the
// slot count, (size_t)-1 beyond the kernels' 32-bit slot index.
template <class Len>
size_t plan_chunks(size_t n, uint32_t* chunk_base, uint32_t* chunk_range, Len len) {
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t c = (len(i) + lzgpu::kCrcChunk - 1) / lzgpu::kCrcChunk;
    if (total + c > 0xFFFFFFFFull) return size_t(-1);
    if (chunk_base) chunk_base[i] = uint32_t(total);
    if (chunk_range)
      for (uint64_t k = 0; k < c; ++k) chunk_range[total + k] = uint32_t(i);
    total += c;
  }
  return size_t(total);
}

}  // namespace

size_t CrcGpu_PlanChunks(const uint64_t* caps, size_t n, uint32_t* chunk_base,
                         uint32_t* chunk_range) {
  return plan_chunks(n, chunk_base, chunk_range, [&](size_t i) { return caps[i]; });
}

size_t LzmaGpu_Crc32Plan(const LzmaGpuStreamDesc* descs, size_t n, uint32_t* chunk_base,
                         uint32_t* chunk_range) {
  return plan_chunks(n, chunk_base, chunk_range, [&](size_t i) { return descs[i].dst_cap; });
}

SRes CrcGpu_Batch(const Byte* d_data, const uint64_t* d_off, const uint64_t* d_len, size_t n,
                  const uint32_t* d_chunk_base, const uint32_t* d_chunk_range, size_t n_chunks,
                  uint32_t init, uint32_t xorout, uint32_t* d_chunk_crc, uint32_t* d_crc,
                  void* stream) {
  return batch_launch("CRC", std::max(n, n_chunks), [&]() {
    return lzgpu_launch_crc_arrays(d_data, d_off, d_len, uint32_t(n), d_chunk_base, d_chunk_range,
                                   uint32_t(n_chunks), init, xorout, d_chunk_crc, d_crc,
                                   static_cast<hipStream_t>(stream));
  });
}

SRes LzmaGpu_Crc32Batch(const LzmaGpuStreamDesc* d_descs, const LzmaGpuResult* d_results,
                        size_t n, const Byte* d_dst, const uint32_t* d_chunk_base,
                        const uint32_t* d_chunk_range, size_t n_chunks, uint32_t* d_chunk_crc,
                        uint32_t* d_crc, void* stream) {
  return batch_launch("CRC", std::max(n, n_chunks), [&]() {
    return lzgpu_launch_crc_decoded(d_descs, d_results, d_dst, uint32_t(n), d_chunk_base,
                                    d_chunk_range, uint32_t(n_chunks), d_chunk_crc, d_crc,
                                    static_cast<hipStream_t>(stream));
  });
}

SRes Crc64Gpu_Batch(const Byte* d_data, const uint64_t* d_off, const uint64_t* d_len, size_t n,
                    const uint32_t* d_chunk_base, const uint32_t* d_chunk_range, size_t n_chunks,
                    uint64_t init, uint64_t xorout, uint64_t* d_chunk_crc, uint64_t* d_crc,
                    void* stream) {
  return batch_launch("CRC-64", std::max(n, n_chunks), [&]() {
    return lzgpu_launch_crc64_arrays(d_data, d_off, d_len, uint32_t(n), d_chunk_base,
                                     d_chunk_range, uint32_t(n_chunks), init, xorout, d_chunk_crc,
                                     d_crc, static_cast<hipStream_t>(stream));
  });
}

// 7zCrc.h drop-ins over host buffers (upload + the batch kernels, n = 1), each
// call on its own stream from the scratch pool: concurrent callers do not
// serialise on the null stream.
void CrcGenerateTable(void) {}  // tables are compile-time constants on the device

static uint32_t crc_host_one(uint32_t init, const void* data, size_t size, uint32_t xorout) {
  if (!ensure_device()) return 0;
  if (size == 0) return init ^ xorout;
  CallScratch* S = scratch_acquire();
  if (!S) return 0;
  const uint64_t cap = size;
  const size_t nch = CrcGpu_PlanChunks(&cap, 1, nullptr, nullptr);
  // one upload: [offset, length | chunk base | chunk ranges]
  std::vector<uint32_t> meta(4 + 1 + nch, 0);
  meta[2] = uint32_t(cap);
  meta[3] = uint32_t(cap >> 32);
  CrcGpu_PlanChunks(&cap, 1, meta.data() + 4, meta.data() + 5);
  uint8_t* d_data = static_cast<uint8_t*>(S->buf[0].get(size));
  uint8_t* d_meta = static_cast<uint8_t*>(S->buf[1].get(4 * meta.size() + 8));
  uint32_t* d_chunks = static_cast<uint32_t*>(S->buf[2].get(4 * (nch + 1)));
  uint32_t out = 0;
  const hipStream_t st = S->stream;
  if (!d_data || !d_meta || !d_chunks) {
    set_error("CRC: device allocation failed");
  } else {
    uint64_t* d_ol = reinterpret_cast<uint64_t*>(d_meta);
    uint32_t* d_base = reinterpret_cast<uint32_t*>(d_meta + 16);
    uint32_t* d_crc = reinterpret_cast<uint32_t*>(d_meta + 4 * meta.size());
    if (hip_ok(hipMemcpyAsync(d_data, data, size, hipMemcpyHostToDevice, st), "CRC H2D") &&
        hip_ok(hipMemcpyAsync(d_meta, meta.data(), 4 * meta.size(), hipMemcpyHostToDevice, st),
               "CRC H2D") &&
        lzgpu_launch_crc_arrays(d_data, d_ol, d_ol + 1, 1, d_base, d_base + 1, uint32_t(nch), init,
                                xorout, d_chunks, d_crc, st) == 0 &&
        hip_ok(hipMemcpyAsync(&out, d_crc, 4, hipMemcpyDeviceToHost, st), "CRC D2H") &&
        hip_ok(hipStreamSynchronize(st), "CRC kernel")) {
    } else {
      out = 0;
    }
  }
  (void)hipStreamSynchronize(st);  // host buffers are reused after return
  scratch_release(S);
  return out;
}

UInt32 CrcUpdate(UInt32 v, const void* data, size_t size) { return crc_host_one(v, data, size, 0); }

UInt32 CrcCalc(const void* data, size_t size) {
  return crc_host_one(0xFFFFFFFFu, data, size, 0xFFFFFFFFu);
}

UInt64 Crc64Calc(const void* data, size_t size) {
  if (!ensure_device()) return 0;
  if (size == 0) return 0;
  DevArr<Byte> d;
  RangeChecks c;
  uint64_t out = 0;
  if (alloc_all("Crc64Calc", d, size) != SZ_OK ||
      !hip_ok(hipMemcpy(d.p, data, size, hipMemcpyHostToDevice), "CRC-64 H2D") ||
      c.prepare("Crc64Calc", 8, {0}, {uint64_t(size)}) != SZ_OK || c.launch(d.p) != SZ_OK ||
      !hip_ok(hipDeviceSynchronize(), "CRC-64 kernel") || !c.fetch(&out, "CRC-64 D2H"))
    return 0;
  return out;
}

// ------------------------------------------------------------------ filters

SRes BcjGpu_X86Batch(Byte* d_data, const uint64_t* d_off, const uint64_t* d_len,
                     const uint32_t* d_ip, uint32_t* d_state, uint64_t* d_done, size_t n,
                     int encoding, void* stream) {
  return batch_launch("BCJ", n, [&]() {
    return lzgpu_launch_bcj_x86(d_data, d_off, d_len, d_ip, d_state, d_done, uint32_t(n), encoding,
                                static_cast<hipStream_t>(stream));
  });
}

SRes BraGpu_Batch(unsigned kind, Byte* d_data, const uint64_t* d_off, const uint64_t* d_len,
                  const uint32_t* d_ip, uint64_t* d_done, size_t n, int encoding, void* stream) {
  if (kind < 5 || kind > 9) return SZ_ERROR_UNSUPPORTED;  // PPC, IA64, ARM, ARMT, SPARC
  return batch_launch("branch converter", n, [&]() {
    return lzgpu_launch_bra(kind, d_data, d_off, d_len, d_ip, d_done, uint32_t(n), encoding,
                            static_cast<hipStream_t>(stream));
  });
}

SRes DeltaGpu_Batch(Byte* d_data, const uint64_t* d_off, const uint64_t* d_len,
                    const uint32_t* d_delta, Byte* d_state, size_t n, int encoding, void* stream) {
  return batch_launch("delta", n, [&]() {
    return lzgpu_launch_delta(d_data, d_off, d_len, d_delta, d_state, uint32_t(n), encoding,
                              static_cast<hipStream_t>(stream));
  });
}

SRes Bcj2Gpu_Batch(const Bcj2GpuJob* d_jobs, size_t n, int32_t* d_res, void* stream) {
  return batch_launch("BCJ2", n, [&]() {
    return lzgpu_launch_bcj2(d_jobs, uint32_t(n), d_res, static_cast<hipStream_t>(stream));
  });
}

namespace {

// One filter over a host buffer: the bytes go up, queue_filter runs the one
// range [0, size) on the null stream, the bytes come back.  fetch(job) reads
// what the drop-in returns beside the data.
template <class Fetch>
bool filter_host(const char* what, const char* name, uint32_t kind, Byte* data, SizeT size,
                 uint32_t prop, int encoding, const uint32_t* x86_state, const Byte* delta_state,
                 Fetch fetch) {
  return guarded("filter: host allocation failed", [&]() -> SRes {
    DevArr<Byte> d;
    FilterJob job;
    const bool ok =
        alloc_all(what, d, size) == SZ_OK &&
        (size == 0 || hip_ok(hipMemcpy(d.p, data, size, hipMemcpyHostToDevice), name)) &&
        queue_filter(what, job, kind, d.p, {0}, {uint64_t(size)}, &prop, encoding, x86_state,
                     delta_state) == SZ_OK &&
        hip_ok(hipDeviceSynchronize(), name) &&
        (size == 0 || hip_ok(hipMemcpy(data, d.p, size, hipMemcpyDeviceToHost), name)) &&
        fetch(job);
    return ok ? SZ_OK : SZ_ERROR_FAIL;
  }) == SZ_OK;
}

// one RISC converter over a host buffer
SizeT bra_convert_host(unsigned kind, const char* name, Byte* data, SizeT size, UInt32 ip,
                       int encoding) {
  if (!ensure_device()) return 0;
  if (size < (kind == 6 ? 16u : 4u)) return 0;
  uint64_t done = 0;
  if (!filter_host("Bra converter", name, kind, data, size, ip, encoding, nullptr, nullptr,
                   [&](FilterJob& j) { return j.fetch_done(&done, name); }))
    return 0;
  return SizeT(done);
}

void delta_host(Byte* state, unsigned delta, Byte* data, SizeT size, int encoding) {
  if (!ensure_device()) return;
  if (delta == 0 || delta > 256) {
    set_error("Delta: delta outside 1..256");
    return;
  }
  Byte st[256] = {0};  // the kernel's state slot; the filter owns its first `delta` bytes
  memcpy(st, state, delta);
  (void)filter_host("Delta", "Delta", 3, data, size, delta, encoding, nullptr, st,
                    [&](FilterJob& j) { return j.fetch_delta_state(state, delta, "Delta D2H"); });
}

}  // namespace

SizeT x86_Convert(Byte* data, SizeT size, UInt32 ip, UInt32* state, int encoding) {
  if (!ensure_device()) return 0;
  if (size < 5) return 0;
  uint64_t done = 0;
  uint32_t st = 0;
  if (!filter_host("x86_Convert", "x86_Convert", 4, data, size, ip, encoding, state, nullptr,
                   [&](FilterJob& j) {
                     return j.fetch_done(&done, "x86_Convert D2H") &&
                            j.fetch_x86_state(&st, "x86_Convert D2H");
                   }))
    return 0;
  *state = st;
  return SizeT(done);
}

SizeT ARM_Convert(Byte* data, SizeT size, UInt32 ip, int encoding) {
  return bra_convert_host(7, "ARM_Convert", data, size, ip, encoding);
}
SizeT ARMT_Convert(Byte* data, SizeT size, UInt32 ip, int encoding) {
  return bra_convert_host(8, "ARMT_Convert", data, size, ip, encoding);
}
SizeT PPC_Convert(Byte* data, SizeT size, UInt32 ip, int encoding) {
  return bra_convert_host(5, "PPC_Convert", data, size, ip, encoding);
}
SizeT SPARC_Convert(Byte* data, SizeT size, UInt32 ip, int encoding) {
  return bra_convert_host(9, "SPARC_Convert", data, size, ip, encoding);
}
SizeT IA64_Convert(Byte* data, SizeT size, UInt32 ip, int encoding) {
  return bra_convert_host(6, "IA64_Convert", data, size, ip, encoding);
}
void Delta_Init(Byte* state) { memset(state, 0, 256); }
void Delta_Encode(Byte* state, unsigned delta, Byte* data, SizeT size) {
  delta_host(state, delta, data, size, 1);
}
void Delta_Decode(Byte* state, unsigned delta, Byte* data, SizeT size) {
  delta_host(state, delta, data, size, 0);
}

// ------------------------------------------------------------------ BCJ2 decode

// Bcj2_Decode over host buffers: the four streams and the output go to the
// device (buf0 inside outBuf, as 7zDec.c:367-372 places it, stays inside the
// device copy of outBuf at the same offset), one lane decodes, the output
// comes back.
static int bcj2_host(const Byte* buf0, SizeT size0, const Byte* buf1, SizeT size1,
                     const Byte* buf2, SizeT size2, const Byte* buf3, SizeT size3, Byte* outBuf,
                     SizeT outSize) {
  if (!ensure_device()) return SZ_ERROR_FAIL;
  const uintptr_t o0 = uintptr_t(outBuf), o1 = o0 + outSize, b0 = uintptr_t(buf0);
  const bool inside = size0 && b0 >= o0 && b0 < o1;
  // device layout: [out (+ main tail beyond it) | buf0 | buf1 | buf2 | buf3]
  const uint64_t out_room = inside ? std::max<uint64_t>(outSize, (b0 - o0) + size0) : outSize;
  const uint64_t off0 = out_room, off1 = off0 + (inside ? 0 : size0), off2 = off1 + size1,
                 off3 = off2 + size2, total = off3 + size3;
  DevArr<Byte> d;
  DevArr<Bcj2GpuJob> dj;
  DevArr<int32_t> dr;
  const SRes ar = alloc_all("Bcj2_Decode", d, size_t(total), dj, 1, dr, 1);
  if (ar != SZ_OK) return ar;
  auto up = [&](uint64_t at, const Byte* p, uint64_t n) {
    return n == 0 || hip_ok(hipMemcpy(d.p + at, p, size_t(n), hipMemcpyHostToDevice), "Bcj2 H2D");
  };
  bool ok = true;
  if (inside) {
    // the host bytes of outBuf (main stream included) and any main tail beyond it
    ok = up(0, outBuf, outSize);
    if (ok && (b0 - o0) + size0 > outSize)
      ok = up(outSize, reinterpret_cast<const Byte*>(o1), (b0 - o0) + size0 - outSize);
  } else {
    // bytes the decoder does not write (an error exit) keep the caller's values
    ok = up(0, outBuf, outSize) && up(off0, buf0, size0);
  }
  ok = ok && up(off1, buf1, size1) && up(off2, buf2, size2) && up(off3, buf3, size3);
  if (!ok) return SZ_ERROR_FAIL;
  Bcj2GpuJob j;
  j.buf0 = inside ? d.p + (b0 - o0) : d.p + off0;
  j.buf1 = d.p + off1;
  j.buf2 = d.p + off2;
  j.buf3 = d.p + off3;
  j.size0 = size0;
  j.size1 = size1;
  j.size2 = size2;
  j.size3 = size3;
  j.out = d.p;
  j.out_size = outSize;
  int32_t r = SZ_ERROR_FAIL;
  if (!hip_ok(hipMemcpy(dj.p, &j, sizeof j, hipMemcpyHostToDevice), "Bcj2 H2D") ||
      Bcj2Gpu_Batch(dj.p, 1, dr.p, nullptr) != SZ_OK || !hip_ok(hipDeviceSynchronize(), "Bcj2") ||
      !hip_ok(hipMemcpy(&r, dr.p, 4, hipMemcpyDeviceToHost), "Bcj2 D2H") ||
      (outSize && !hip_ok(hipMemcpy(outBuf, d.p, outSize, hipMemcpyDeviceToHost), "Bcj2 D2H")))
    return SZ_ERROR_FAIL;
  return r;
}

int Bcj2_Decode(const Byte* buf0, SizeT size0, const Byte* buf1, SizeT size1, const Byte* buf2,
                SizeT size2, const Byte* buf3, SizeT size3, Byte* outBuf, SizeT outSize) {
  return guarded("Bcj2_Decode: host allocation failed", [&]() {
    return bcj2_host(buf0, size0, buf1, size1, buf2, size2, buf3, size3, outBuf, outSize);
  });
}

// ------------------------------------------------------------------ SHA-256

// The Sha256.h drop-ins over host buffers and the batch form over device
// ranges; a drop-in call runs on its own stream from the scratch pool, like
// the CRC-32 ones.  No compression function lives on the host: it
// buffers bytes until a block is complete, as Sha256_Update does
// (Sha256.c:160-174), and every block, the padding blocks included, is
// compressed by lzgpu_launch_sha256 (sha256_kernels.hip).
static_assert(sizeof(CSha256) == 104, "CSha256 layout (Sha256.h:13-18)");

// The kernels' translation unit is part of the library.  A host-only link of
// the container parsers that leaves it out (the sanitizer build of
// tests/fuzz/) still links: the reference is weak, and a call without the
// kernels is an error, never a host computation.
extern "C" __attribute__((weak)) int lzgpu_launch_sha256(
    const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_len, uint32_t n,
    const uint32_t* d_init, const uint64_t* d_prior, int finalise, unsigned kernel,
    uint8_t* d_out, hipStream_t stream);

static int sha256_launch(const uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_len,
                         uint32_t n, const uint32_t* d_init, const uint64_t* d_prior,
                         int finalise, unsigned kernel, uint8_t* d_out, hipStream_t stream) {
  if (!lzgpu_launch_sha256) return -3;
  return lzgpu_launch_sha256(d_data, d_off, d_len, n, d_init, d_prior, finalise, kernel, d_out,
                             stream);
}

SRes Sha256Gpu_Batch(const Byte* d_data, const uint64_t* d_off, const uint64_t* d_len, size_t n,
                     unsigned kernel, Byte* d_digest, void* stream) {
  if (kernel > LZMA_GPU_SHA256_WAVE || n > 0xFFFFFFFFull) return SZ_ERROR_PARAM;
  return batch_launch("SHA-256", n, [&]() {
    return sha256_launch(d_data, d_off, d_len, uint32_t(n), nullptr, nullptr, 1, kernel, d_digest,
                         static_cast<hipStream_t>(stream));
  });
}

namespace {

// One range on the device: head (the bytes buffered in the struct) followed by
// body, continued from `state` with `prior` bytes hashed before.  finalise:
// out = the 32 digest bytes; else out = the state after the whole blocks.
// One message is one serial chain: the wave kernel.
bool sha256_host_range(const uint32_t state[8], uint64_t prior, const Byte* head, size_t n_head,
                       const Byte* body, size_t n_body, int finalise, void* out) {
  lzgpu_host::CallScratch* S = lzgpu_host::scratch_acquire();
  if (!S) return false;
  const size_t size = n_head + n_body;
  // one upload: [offset, length, prior | state | 32 bytes of result]
  uint64_t meta[3 + 4] = {0, uint64_t(size), prior};
  memcpy(meta + 3, state, 32);
  uint8_t* d_data = static_cast<uint8_t*>(S->buf[0].get(size));
  uint8_t* d_meta = static_cast<uint8_t*>(S->buf[1].get(sizeof meta + 32));
  const hipStream_t st = S->stream;
  bool ok = false;
  if (!d_data || !d_meta) {
    set_error("SHA-256: device allocation failed");
  } else {
    uint64_t* d_m = reinterpret_cast<uint64_t*>(d_meta);
    ok = (n_head == 0 ||
          hip_ok(hipMemcpyAsync(d_data, head, n_head, hipMemcpyHostToDevice, st), "SHA-256 H2D")) &&
         (n_body == 0 || hip_ok(hipMemcpyAsync(d_data + n_head, body, n_body,
                                               hipMemcpyHostToDevice, st),
                                "SHA-256 H2D")) &&
         hip_ok(hipMemcpyAsync(d_meta, meta, sizeof meta, hipMemcpyHostToDevice, st),
                "SHA-256 H2D");
    if (ok && sha256_launch(d_data, d_m, d_m + 1, 1, reinterpret_cast<uint32_t*>(d_m + 3),
                                  d_m + 2, finalise, kLzgpuSha256Wave, d_meta + sizeof meta,
                                  st) != 0) {
      set_error("SHA-256 kernel launch failed");
      ok = false;
    }
    ok = ok &&
         hip_ok(hipMemcpyAsync(out, d_meta + sizeof meta, 32, hipMemcpyDeviceToHost, st),
                "SHA-256 D2H") &&
         hip_ok(hipStreamSynchronize(st), "SHA-256 kernel");
  }
  (void)hipStreamSynchronize(st);  // host buffers are reused after return
  lzgpu_host::scratch_release(S);
  return ok;
}

}  // namespace

void Sha256_Init(CSha256* p) {
  static const UInt32 iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                               0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  memcpy(p->state, iv, sizeof iv);
  p->count = 0;
}

void Sha256_Update(CSha256* p, const Byte* data, size_t size) {
  const size_t fill = size_t(p->count & 0x3F);
  if (size < 64 - fill) {  // no block completes: buffer only
    if (size) memcpy(p->buffer + fill, data, size);
    p->count += size;
    return;
  }
  // the buffered bytes and the data up to the last block boundary go to the
  // device; what is left over becomes the new buffer contents
  const size_t whole = ((fill + size) & ~size_t(63)) - fill, rest = size - whole;
  if (ensure_device()) {
    UInt32 st[8];
    if (sha256_host_range(p->state, p->count - fill, p->buffer, fill, data, whole, 0, st))
      memcpy(p->state, st, sizeof st);
  }
  if (rest) memcpy(p->buffer, data + whole, rest);
  p->count += size;
}

void Sha256_Final(CSha256* p, Byte* digest) {
  const size_t fill = size_t(p->count & 0x3F);
  if (!ensure_device() ||
      !sha256_host_range(p->state, p->count - fill, p->buffer, fill, nullptr, 0, 1, digest))
    memset(digest, 0, SHA256_DIGEST_SIZE);
  Sha256_Init(p);
}
