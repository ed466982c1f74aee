// lzmaenc_session_kernels.hip -- one round of LZMA encoder sessions for gfx950:
// every session of a batch makes one LzmaEnc::session_call (lzmaenc_device.h) on
// the stream it has been given so far, with its encoder resident in the
// LzmaEncGpuSession record and its tables in its workspace slice.
//
//   lzmaenc_session_list_kernel    over all n records: the indices of those with
//                          work this round (lzenc::session_has_work) are
//                          compacted onto scratch's work list, those of them
//                          whose slice still needs initialising onto its init
//                          list: a ballot per wave, one atomic per wave and
//                          list, the lane's place from the prefix count.  The
//                          order within a list is that of the waves' atomics.
//   lzmaenc_session_init_kernel    the whole grid over the init list, as
//                          lzmaenc_init_kernel is over streams: hash clear and
//                          cells to kProbInit, (session, part) pairs dealt over
//                          the workgroups.  The count is read on the device.
//   lzmaenc_session_encode_kernel  the fast kernel's geometry: one wave per
//                          workgroup, `lanes` sessions per wave, the CRC table
//                          in LDS.  The grid is ceil(n / lanes) whatever the
//                          round holds; a workgroup past the work list returns
//                          before it builds the table, so a round in which 1 %
//                          of the sessions have input occupies 1 % of the waves.
//                          The state goes back to the record with ordinary
//                          stores.
// A session without work is read by the list pass alone and written by nobody.
//
// ReadMatchDistances is a real call in this translation unit
// (LZENC_DEVICE_NOINLINE), as in the normal-mode kernels and for their reason
// ("Open defect"): with every function inlined at -O3 the encode
// kernel below (110 VGPRs, no scratch) gave 45 of the 200 streams of
// tests/test_lzmaenc_session_gpu.py other bytes than the one-shot kernel, in a
// single final call already, identically on every run; this build, and an -O1
// build, give the one-shot kernel's bytes for every stream and schedule.
#define LZENC_DEVICE_NOINLINE 1
#include <hip/hip_runtime.h>

#include "../../include/lzma_gpu.h"
#include "lzmaenc_device.h"
#include "lzmaenc_internal.h"

namespace {

constexpr uint32_t kListThreads = 256, kInitThreads = 256;

// this lane's place among the set bits of a wave's ballot
__device__ __forceinline__ uint32_t prefix_of(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
}
// appends `id` to list[] for every lane with take set; the wave's first lane
// reserves the room.  Called by all 64 lanes of a wave.
__device__ __forceinline__ void wave_append(bool take, uint32_t id, uint32_t* counter,
                                            uint32_t* list) {
  const uint64_t mask = __ballot(take);
  if (mask == 0) return;
  uint32_t base = 0;
  if ((threadIdx.x & 63u) == 0) base = atomicAdd(counter, uint32_t(__popcll(mask)));
  base = __shfl(base, 0);
  if (take) list[base + prefix_of(mask)] = id;
}

__global__ void __launch_bounds__(kListThreads) lzmaenc_session_list_kernel(
    const LzmaEncGpuSession* __restrict__ sessions, uint32_t n, uint32_t* __restrict__ scratch) {
  const uint64_t i = uint64_t(blockIdx.x) * kListThreads + threadIdx.x;
  bool work = false, init = false;
  if (i < n) {
    const LzmaEncGpuSession& s = sessions[i];
    work = lzenc::session_has_work(s, lzenc::kSessionHold);
    init = work && lzenc::session_wants_init(s, lzenc::kSessionHold);
  }
  wave_append(work, uint32_t(i), scratch + kLzmaEncSessionWorkCount,
              scratch + kLzmaEncSessionHeaderWords);
  wave_append(init, uint32_t(i), scratch + kLzmaEncSessionInitCount,
              scratch + kLzmaEncSessionHeaderWords + n);
}

__global__ void __launch_bounds__(kInitThreads) lzmaenc_session_init_kernel(
    const LzmaEncGpuSession* __restrict__ sessions, uint32_t n,
    const uint32_t* __restrict__ scratch) {
  const uint32_t count = scratch[kLzmaEncSessionInitCount];
  if (count == 0 || count > n) return;
  // as lzmaencgpu_launch_init: about 4,096 workgroups' worth of parts, at most 64 a slice
  uint32_t parts = (4096 + count - 1) / count;
  if (parts > 64) parts = 64;
  const uint32_t* list = scratch + kLzmaEncSessionHeaderWords + n;
  const uint64_t total = uint64_t(count) * parts;
  for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint32_t id = list[w / parts], part = uint32_t(w % parts);
    if (id >= n) continue;
    const LzmaEncGpuSession& s = sessions[id];
    const lzenc::Layout l = lzenc::lzmaenc_layout(lzenc::session_params(s), s.src_cap);
    lzenc::lzmaenc_init_slice(static_cast<uint8_t*>(s.ws), l,
                              uint64_t(part) * kInitThreads + threadIdx.x,
                              uint64_t(parts) * kInitThreads);
  }
}

__global__ void __launch_bounds__(64) lzmaenc_session_encode_kernel(
    LzmaEncGpuSession* __restrict__ sessions, uint32_t n, uint32_t lanes,
    const uint32_t* __restrict__ scratch) {
  uint32_t count = scratch[kLzmaEncSessionWorkCount];
  if (count > n) count = n;
  if (uint64_t(blockIdx.x) * lanes >= count) return;
  __shared__ uint32_t crc[256];
  for (uint32_t v = threadIdx.x; v < 256; v += 64) crc[v] = lzenc::crc_entry(v);
  __syncthreads();
  if (threadIdx.x >= lanes) return;
  const uint64_t k = uint64_t(blockIdx.x) * lanes + threadIdx.x;
  if (k >= count) return;
  const uint32_t id = scratch[kLzmaEncSessionHeaderWords + k];
  if (id >= n) return;
  lzenc::LzmaEnc e;
  e.session_call(sessions[id], crc, lzenc::kSessionHold);
}

}  // namespace

extern "C" int lzmaencgpu_session_launch_list(const LzmaEncGpuSession* d_sessions, uint32_t n,
                                              uint32_t* d_scratch, hipStream_t stream) {
  if (n == 0) return 0;
  if (hipMemsetAsync(d_scratch, 0, kLzmaEncSessionHeaderWords * 4, stream) != hipSuccess) return -1;
  hipLaunchKernelGGL(lzmaenc_session_list_kernel, dim3((n + kListThreads - 1) / kListThreads),
                     dim3(kListThreads), 0, stream, d_sessions, n, d_scratch);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzmaencgpu_session_launch(LzmaEncGpuSession* d_sessions, uint32_t n,
                                         uint32_t* d_scratch, uint32_t lanes, hipStream_t stream) {
  if (n == 0) return 0;
  if (lanes != 0 && lanes != 16 && lanes != 32 && lanes != 64) return -2;
  if (lzmaencgpu_session_launch_list(d_sessions, n, d_scratch, stream) != 0) return -1;
  const uint64_t want = uint64_t(n) * 64;
  hipLaunchKernelGGL(lzmaenc_session_init_kernel, dim3(uint32_t(want < 65536 ? want : 65536)),
                     dim3(kInitThreads), 0, stream, d_sessions, n, d_scratch);
  if (hipGetLastError() != hipSuccess) return -1;
  const uint32_t lf = lanes ? lanes : kLzmaEncLanesDefault;
  const uint32_t groups = uint32_t((uint64_t(n) + lf - 1) / lf);
  hipLaunchKernelGGL(lzmaenc_session_encode_kernel, dim3(groups), dim3(64), 0, stream, d_sessions,
                     n, lf, d_scratch);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
