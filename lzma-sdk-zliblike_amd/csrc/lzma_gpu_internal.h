// lzma_gpu_internal.h -- kernel launch entry points used by the host C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "decode_plan.h"
#include "lzma_lane.h"

// Devices the library keeps per-device state for (launch attributes, class
// streams, CU counts, dictionary mirrors).
constexpr int kLzgpuMaxDevices = 64;

extern "C" int lzgpu_launch_decode_batch(const LzmaGpuStreamDesc* d_descs, const uint32_t* d_order,
                                         uint32_t n, const uint8_t* d_src, uint8_t* d_dst,
                                         uint16_t* d_ws, LzmaGpuResult* d_results,
                                         hipStream_t stream);
extern "C" int lzgpu_launch_session(LzgpuSession* d_sess, uint32_t n, hipStream_t stream);
// cooperative sessions: one 32-lane wave per session, tables of at most
// lds_cells cells staged in LDS for the call; max_groups 0 = one per session
extern "C" int lzgpu_launch_session_coop(LzgpuSession* d_sess, uint32_t n, uint32_t lds_cells,
                                         uint32_t max_groups, hipStream_t stream);
// lets a kernel launch with up to 160 KiB of dynamic LDS (once per kernel and
// device, thread-safe); 0 on success
int lzgpu_allow_full_lds(const void* kfn);
// largest table (cells) the cooperative session kernel stages in LDS: lc+lp <= 4
// at any pb (LZMA2's bound, 28 KiB) and wider LZMA tables up to 64 KiB
constexpr uint32_t kSessCoopMaxCells = 32768;
// One LDS class of a plan (c.n streams; order and queue the class's own) with the
// kernel and launch shape decode_plan.h gives it, at most max_groups workgroups
// (0 = no cap).  -1: no kernel is built for the class, or the launch failed.
struct LzgpuDecodeBufs {
  const LzmaGpuStreamDesc* descs;
  const uint32_t* order;
  const uint8_t* src;
  uint8_t* dst;
  uint16_t* ws;
  LzmaGpuResult* results;
  uint32_t* queue;
};
extern "C" int lzgpu_launch_decode_lds(const LzmaGpuLdsClass& c, const LzgpuDecodeBufs& b,
                                       uint32_t max_groups, hipStream_t stream);
// The launchers' own shapes, for tests (cus 0 = the current device's, env null =
// the process's LZGPU_DUP / LZGPU_WIN): 1 = *out filled, 0 = no kernel.
extern "C" int lzgpu_decode_launch_shape(const LzmaGpuLdsClass* c, uint32_t n, uint32_t max_groups,
                                         uint32_t cus, const lzgpu_host::LaunchEnv* env,
                                         lzgpu_host::LaunchShape* out);
extern "C" int lzgpu_session_launch_shape(uint32_t n, uint32_t lds_cells, uint32_t max_groups,
                                          uint32_t cus, const lzgpu_host::LaunchEnv* env,
                                          lzgpu_host::LaunchShape* out);
// rows[4 i ..] = (family, w, mask, k2) of kernel table row i < cap; returns the row count
extern "C" uint32_t lzgpu_decode_kernel_rows(uint32_t* rows, uint32_t cap);
// ---- the range primitives (range_capi.hip), 0 on success.  CRC-32 / CRC-64
// (crc_kernels.hip) over arrays of ranges or a decode batch's own results
extern "C" int lzgpu_launch_crc_arrays(const uint8_t* d_data, const uint64_t* d_off,
                                       const uint64_t* d_len, uint32_t n,
                                       const uint32_t* d_chunk_base,
                                       const uint32_t* d_chunk_range, uint32_t n_chunks,
                                       uint32_t init, uint32_t xorout, uint32_t* d_chunk_crc,
                                       uint32_t* d_crc, hipStream_t stream);
extern "C" int lzgpu_launch_crc_decoded(const LzmaGpuStreamDesc* d_descs,
                                        const LzmaGpuResult* d_results, const uint8_t* d_dst,
                                        uint32_t n, const uint32_t* d_chunk_base,
                                        const uint32_t* d_chunk_range, uint32_t n_chunks,
                                        uint32_t* d_chunk_crc, uint32_t* d_crc,
                                        hipStream_t stream);
extern "C" int lzgpu_launch_crc64_arrays(const uint8_t* d_data, const uint64_t* d_off,
                                         const uint64_t* d_len, uint32_t n,
                                         const uint32_t* d_chunk_base,
                                         const uint32_t* d_chunk_range, uint32_t n_chunks,
                                         uint64_t init, uint64_t xorout, uint64_t* d_chunk_crc,
                                         uint64_t* d_crc, hipStream_t stream);
// SHA-256 of n device ranges d_data[off[i] .. off[i] + len[i]) (sha256_kernels.hip),
// the one launcher behind Sha256Gpu_Batch, the Sha256.h drop-ins and the xz
// block check.  Range i continues from the chaining state d_init[8 * i .. + 8)
// (null: the initial value) with d_prior[i] bytes already hashed (null: 0; they
// count in the length field).  finalise != 0: the range is padded and
// d_out[32 * i .. + 32) is its digest; finalise == 0: only its whole 64-byte
// blocks are hashed and d_out holds the eight state words as uint32.
// kernel: lane per range, wave per range, or by n alone (lengths live on the
// device).  0 on success, -2 for an unknown kernel, -1 if the launch failed.
constexpr unsigned kLzgpuSha256Auto = 0, kLzgpuSha256Lane = 1, kLzgpuSha256Wave = 2;
// AUTO takes the lane kernel from this many ranges on: more ranges than the
// chip has SIMDs (256 CUs x 4).  Measured with 1 MiB ranges
// (profiles/sha256/crossover.jsonl): up to 1,024 ranges every wave of the wave
// kernel has a SIMD to itself and a range takes 29.4-29.7 ms against the lane
// kernel's 46.6-51.2 ms; a second wave on a SIMD doubles that (2,048 ranges:
// 56.2 ms, lane 48.8 ms; 4,096: 136 ms, lane 48.9 ms), while the lane kernel's
// time stays flat to 16,384 ranges (49.0 ms).  Not measured between 1,024 and
// 2,048: there some SIMDs already hold two waves, so the batch takes the
// two-wave time.
constexpr uint32_t kLzgpuSha256AutoLaneMin = 1025;
extern "C" int lzgpu_launch_sha256(const uint8_t* d_data, const uint64_t* d_off,
                                   const uint64_t* d_len, uint32_t n, const uint32_t* d_init,
                                   const uint64_t* d_prior, int finalise, unsigned kernel,
                                   uint8_t* d_out, hipStream_t stream);
// the filters (filter_kernels.hip)
extern "C" int lzgpu_launch_bcj_x86(uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_len,
                                    const uint32_t* d_ip, uint32_t* d_state, uint64_t* d_done,
                                    uint32_t n, int encoding, hipStream_t stream);
extern "C" int lzgpu_launch_bra(uint32_t kind, uint8_t* d_data, const uint64_t* d_off,
                                const uint64_t* d_len, const uint32_t* d_ip, uint64_t* d_done,
                                uint32_t n, int encoding, hipStream_t stream);
extern "C" int lzgpu_launch_bcj2(const Bcj2GpuJob* d_jobs, uint32_t n, int32_t* d_res,
                                 hipStream_t stream);
extern "C" int lzgpu_launch_delta(uint8_t* d_data, const uint64_t* d_off, const uint64_t* d_len,
                                  const uint32_t* d_delta, uint8_t* d_state, uint32_t n,
                                  int encoding, hipStream_t stream);

// host-side helpers shared by the C-ABI translation units (defined in lzma_capi.hip)
namespace lzgpu_host {

bool ensure_device();
void set_error(const char* what);
bool hip_ok(hipError_t e, const char* what);
// CUs of the current device once the library has started the HIP runtime
// (ensure_device), else MI355X's 256 without touching the runtime
uint32_t device_cus();

// host CRC-32 for container metadata (7zCrc.c semantics; headers, a few
// bytes per block -- decoded data is checked on the GPU)
inline uint32_t crc32_host(const uint8_t* p, size_t n) {
  static uint32_t t[256];
  static bool init = false;
  if (!init) {
    for (uint32_t v = 0; v < 256; ++v) {
      uint32_t r = v;
      for (int j = 0; j < 8; ++j) r = (r >> 1) ^ ((r & 1u) ? 0xEDB88320u : 0u);
      t[v] = r;
    }
    init = true;
  }
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = t[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

// Grow-only device buffer on one device (per-call scratch of the host-buffer
// entry points; pooled per device, see CallScratch).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  void* get(size_t n) {
    if (n == 0) n = 16;
    if (p && cap >= n) return p;
    size_t want = n > cap * 2 ? n : cap * 2;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      p = nullptr;
      if (hipMalloc(&p, n) != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
        return nullptr;
      }
      want = n;
    }
    cap = want;
    return p;
  }
};

// Scratch of one host-buffer call (LzmaDecode, LzmaUncompress, the CRC
// drop-ins, ...): device buffers plus a non-blocking stream of its own, taken
// from a per-device pool for the call and returned after it.  The pool grows
// to the number of calls in flight at once, not to the number of threads that
// ever called (nothing is thread-local, nothing leaks per thread).
struct CallScratch {
  DevBuf buf[4];
  hipStream_t stream = nullptr;
  int dev = 0;
  uint8_t* pin = nullptr;  // pinned host staging (scratch_pinned)
  size_t pin_cap = 0;
};
CallScratch* scratch_acquire();  // current device; nullptr (error set) on failure
void scratch_release(CallScratch* s);
// The scratch's pinned host staging, at least n bytes (grown geometrically from
// 256 KiB, at most kPinnedStageMax); nullptr when n is larger or the allocation
// fails -- the caller then copies from / to pageable memory directly.  A
// pageable hipMemcpyAsync goes through the runtime's own staging buffer, one
// per device, so concurrent callers' small copies queue behind each other.
constexpr size_t kPinnedStageMax = size_t(8) << 20;
uint8_t* scratch_pinned(CallScratch* s, size_t n);

// owning device array for the container drivers' per-call buffers
template <class T>
struct DevArr {
  T* p = nullptr;
  DevArr() = default;
  DevArr(const DevArr&) = delete;
  DevArr& operator=(const DevArr&) = delete;
  ~DevArr() {
    if (p) (void)hipFree(p);
  }
  bool alloc(size_t n) { return hipMalloc(&p, (n ? n : 1) * sizeof(T)) == hipSuccess; }
};
}  // namespace lzgpu_host
