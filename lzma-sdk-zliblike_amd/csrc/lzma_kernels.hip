// lzma_kernels.hip -- batch LZMA / LZMA2 decode kernels for gfx950.
//
// lzgpu_decode_lds_kernel (fast path, LZMA items whose lo table fits LDS):
//   one stream per lane, L lanes per workgroup (one wave with L active
//   lanes), each lane's lo probability table in its own LDS slice of
//   `stride` cells (L and the workgroups per CU: decode_plan.h).  The
//   hardware dispatcher starts a new workgroup whenever
//   one retires, so a 64K-stream batch streams through the chip in waves of
//   resident workgroups with no host round trips.
// lzgpu_decode_batch_kernel (generic: any lc/lp/pb, LZMA2 ranges): 64 lanes
//   per workgroup, whole table in the item's global workspace slice.
// lzgpu_session_kernel: one LzmaDec_DecodeToDic call per lane on a
//   device-resident decoder state (dictionary / buffer interfaces).
// `order` (optional) maps lane -> descriptor so the planner can put streams of
// similar length into the same wave (a wave runs until its slowest lane ends).
// The per-lane work is in lzma_lane.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <set>
#include <utility>

#include "lzma_gpu_internal.h"

using namespace lzgpu;

// Dynamic-LDS limit of a kernel raised to the CU's 160 KiB once per device
// (the attribute is per device: a process driving several GPUs, or threads
// whose first launches race, each get it set before their launch).
static int allow_full_lds(const void* kfn) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kLzgpuMaxDevices) return -1;
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  std::lock_guard<std::mutex> g(mu);
  if (done.count({kfn, dev})) return 0;
  if (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
      hipSuccess)
    return -1;
  done.insert({kfn, dev});
  return 0;
}

int lzgpu_allow_full_lds(const void* kfn) { return allow_full_lds(kfn); }

__global__ void __launch_bounds__(64) lzgpu_decode_batch_kernel(
    const LzmaGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order, uint32_t n,
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint16_t* __restrict__ ws,
    LzmaGpuResult* __restrict__ results) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  const uint32_t id = order ? order[lane] : lane;
  const LzmaGpuStreamDesc d = descs[id];
  results[id] = lane_decode(d, src, dst, ws);
}

// W = minimum waves per SIMD the register allocation must allow (the
// planner's occupancy target; more resident waves hide the serial decode
// chain of each stream better, at the price of register spills).
// Persistent lanes: the grid is sized to what is resident at once; a lane
// that finishes its stream takes the next one from `queue` (a counter the
// launcher zeroes), so no lane idles behind a slower neighbour in its wave
// and the chip drains without a partial last round of workgroups.  Every
// lane exits once the queue passes n.  Lane l starts on stream l and then
// takes start + (queue ticket): start = the lanes of the launch.
// K2: the build carries the LZMA2 chunk walker (classes with LZMA2 items); the
// LZMA-only build needs fewer registers (169 vs 202 VGPRs at W = 2, 21 vs 153
// spilled at W = 4), so classes without LZMA2 items launch it.
// Lane-interleaved placements (M & kIlvBit): the global sections live in the
// class's slot area (`slot_off` cells into ws) instead of per-stream slices --
// lane group g (32 lanes of one workgroup) owns rows of kIlv cells, `slot_cells`
// rows, and lane l its column l; the lane keeps its column for every stream
// it takes from the queue.

template <int W, uint32_t M, bool K2>
__global__ void __launch_bounds__(64, W) lzgpu_decode_lds_kernel(
    const LzmaGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order, uint32_t n,
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint16_t* __restrict__ ws,
    LzmaGpuResult* __restrict__ results, uint32_t stride, uint32_t* __restrict__ queue,
    uint64_t slot_off, uint32_t slot_cells, uint32_t start) {
  extern __shared__ uint32_t lz_smem[];
  // the lane's LDS slice; interleaved (lds_ilv): its column of its 32-lane
  // group's rows
  lds_u16* lo = (lds_u16*)((uint16_t*)lz_smem);
  if constexpr (lds_ilv<M>())
    lo += (threadIdx.x / kIlv) * (kIlv * stride) + (threadIdx.x % kIlv);
  else
    lo += threadIdx.x * stride;
  uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  gu16* gcol = nullptr;
  if constexpr ((M & kIlvBit) != 0u) {
    const uint32_t grp = blockIdx.x * ((blockDim.x + kIlv - 1) / kIlv) + threadIdx.x / kIlv;
    gcol = (gu16*)(ws + slot_off) + uint64_t(grp) * slot_cells * kIlv +
           (threadIdx.x % kIlv) * kIlvLaneCells;
  }
  (void)slot_off;
  (void)slot_cells;
  while (idx < n) {
    const uint32_t id = order ? order[idx] : idx;
    const LzmaGpuStreamDesc d = descs[id];
    // (W = 4 of the throughput placement: without the round-9 load batches)
    constexpr uint32_t ML = (W > 2 && (M & ~kIlvBit) == LZGPU_LDS_MASK) ? (M | kMpOffBit) : M;
    results[id] = lane_decode_lds<ML, K2>(d, src, dst, ws, lo, stride, gcol);
    idx = start + atomicAdd(queue, 1u);
  }
}

// One-stream waves of the latency placement (round 5): the one-lane decoder
// run by all D lanes of a workgroup on the same stream -- the instruction
// stream of lzgpu_decode_lds_kernel with one lane per wave, but with D >= 16
// lanes in EXEC.  The SIMD issue micro-benchmark (scripts/ubench/
// simd_issue_ubench.hip lanes, profiles/r05_issue/simd_lanes.jsonl) finds a
// VALU instruction of a wave with 1-8 active lanes issuing once per ~16.7
// cycles alone on its SIMD and at 3.5 cycles per SIMD with four such waves,
// against 4.8 / 2.5 cycles with 16 or more lanes; a dependent LDS decision
// chain takes 98 against 75 cycles per SIMD at four waves.  Config 2 6.28 ->
// 6.86 GB/s, config 5 5.13 -> 5.58 (profiles/r05_dup/).  The lanes share the
// workgroup's LDS slice and store identical values to identical addresses;
// lane 0 writes the result and takes the next stream from the queue.
constexpr int kLaneDup = 32;
template <int W, uint32_t M, bool K2>
__global__ void __launch_bounds__(64, W) lzgpu_decode_dup_kernel(
    const LzmaGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order, uint32_t n,
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint16_t* __restrict__ ws,
    LzmaGpuResult* __restrict__ results, uint32_t stride, uint32_t* __restrict__ queue) {
  extern __shared__ uint32_t lz_smem[];
  lds_u16* lo = (lds_u16*)((uint16_t*)lz_smem);
  uint32_t idx = blockIdx.x;
  while (idx < n) {
    const uint32_t id = order ? order[idx] : idx;
    LzmaGpuStreamDesc d = descs[id];
    // keep the shared decoder state in vector registers (lz_vzero)
    const uint32_t z = lz_vzero();
    d.src_off += z;
    d.dst_off += z;
    const LzmaGpuResult r = lane_decode_lds<M | kDupBit, K2>(d, src, dst, ws, lo, stride, nullptr);
    uint32_t next = 0;
    if (threadIdx.x == 0) {
      results[id] = r;
      next = gridDim.x + atomicAdd(queue, 1u);
    }
    idx = uint32_t(__builtin_amdgcn_readfirstlane(int(next)));
  }
}

// Wave-cooperative decode (latency regime): one stream per workgroup of one
// 32-lane wave.  Every lane runs the same decoder on the same state, so control
// flow and memory traffic are those of one lane -- except match copies (byte j
// by lane j mod 32, lz_copy_coop), the direct bits of a distance (several per
// step, direct_coop) and table initialisation.  Lane 0 takes the next stream
// from the queue.
// Under kWinBit the workgroup's LDS holds, after the table (`stride` cells,
// 16-byte aligned), the LDS history window of `win_bytes` (lzma_device.h):
// match copies and matched bytes within its reach are LDS reads.
template <int W, uint32_t M, bool K2>
__global__ void __launch_bounds__(32, W) lzgpu_decode_coop_kernel(
    const LzmaGpuStreamDesc* __restrict__ descs, const uint32_t* __restrict__ order, uint32_t n,
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint16_t* __restrict__ ws,
    LzmaGpuResult* __restrict__ results, uint32_t stride, uint32_t* __restrict__ queue,
    uint32_t win_bytes) {
  extern __shared__ uint32_t lz_smem[];
  lds_u16* lo = (lds_u16*)((uint16_t*)lz_smem);
  lds_u8* win = (lds_u8*)((uint8_t*)lz_smem) + ((size_t(stride) * 2 + 15) & ~size_t(15));
  uint32_t idx = blockIdx.x;
  while (idx < n) {
    const uint32_t id = order ? order[idx] : idx;
    LzmaGpuStreamDesc d = descs[id];
    // keep the shared decoder state in vector registers (lz_vzero)
    const uint32_t z = lz_vzero();
    d.src_off += z;
    d.dst_off += z;
    const LzmaGpuResult r =
        lane_decode_lds<M, K2>(d, src, dst, ws, lo, stride, nullptr, win, win_bytes);
    uint32_t next = 0;
    if (threadIdx.x == 0) {
      results[id] = r;
      next = gridDim.x + atomicAdd(queue, 1u);
    }
    idx = uint32_t(__builtin_amdgcn_readfirstlane(int(next)));
  }
}

// One DecodeToDic call per lane on a device-resident decoder state.
__global__ void __launch_bounds__(64) lzgpu_session_kernel(LzgpuSession* __restrict__ sess,
                                                           uint32_t n) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n) return;
  lane_session(sess[lane]);
}

// One DecodeToDic / DecodeToBuf call per workgroup of one 32-lane wave on a
// device-resident decoder (the drop-in LzmaDec_DecodeToDic / DecodeToBuf of a
// host CLzmaDec, and small session batches): the wave-cooperative decoder with
// the session's whole table staged in LDS for the call -- loaded from
// q.probs, decoded on (every table access an LDS round trip instead of a
// global one), written back.  Placement
// 0x7FF keeps the all-global layout's offsets, so the copy is a straight one.
// Dynamic LDS: the widest table of the batch's sessions (the launcher checks).
// WIN: the LDS history window (win_bytes, after the table) is preloaded per
// call with the dictionary bytes a match can reach (lane_session).
constexpr uint32_t kSessCoopMask = LZGPU_LDS_MASK_ALL | kCoopBit;
template <bool WIN>
__global__ void __launch_bounds__(32) lzgpu_session_coop_kernel(LzgpuSession* __restrict__ sess,
                                                                 uint32_t n, uint32_t lds_cells,
                                                                 uint32_t win_bytes) {
  extern __shared__ uint32_t lz_smem[];
  lds_u16* lo = (lds_u16*)((uint16_t*)lz_smem);
  lds_u8* win = (lds_u8*)((uint8_t*)lz_smem) + ((size_t(lds_cells) * 2 + 15) & ~size_t(15));
  constexpr uint32_t MS = kSessCoopMask | (WIN ? kWinBit : 0u);
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    LzgpuSession q = sess[i];
    // keep the shared decoder state in vector registers (lz_vzero)
    {
      const uint32_t z = lz_vzero();
      q.in = (const uint8_t*)q.in + z;
      q.dic = (uint8_t*)q.dic + z;
    }
    const uint32_t cells = table_cells(q.lc, q.lp, q.pb);
    if (cells > lds_cells) {  // planned for narrower tables: refuse, state untouched
      if (threadIdx.x == 0) {
        sess[i].res = kErrMem;
        sess[i].status = kStNone;
      }
      continue;
    }
    gu16* gp = (gu16*)q.probs;
    for (uint32_t j = threadIdx.x; j < cells; j += blockDim.x) lo[j] = gp[j];
    __syncthreads();
    lane_session<MS>(q, lo, win, win_bytes);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < cells; j += blockDim.x) gp[j] = lo[j];
    if (threadIdx.x == 0) sess[i] = q;
    __syncthreads();
  }
}

// LZGPU_DUP=D (A/B; D = 1 launches the one-lane kernel) and LZGPU_WIN=0 (no LDS
// history window), read once per process
static const lzgpu_host::LaunchEnv& launch_env() {
  static const lzgpu_host::LaunchEnv env = [] {
    const char *d = getenv("LZGPU_DUP"), *w = getenv("LZGPU_WIN");
    return lzgpu_host::LaunchEnv{d ? atoi(d) : kLaneDup, (w && w[0] == '0') ? 1u : 0u};
  }();
  return env;
}

extern "C" int lzgpu_session_launch_shape(uint32_t n, uint32_t lds_cells, uint32_t max_groups,
                                          uint32_t cus, const lzgpu_host::LaunchEnv* env,
                                          lzgpu_host::LaunchShape* out) {
  return lzgpu_host::session_launch_shape(n, lds_cells, max_groups,
                                          cus ? cus : lzgpu_host::device_cus(),
                                          env ? *env : launch_env(), *out);
}

extern "C" int lzgpu_launch_session_coop(LzgpuSession* d_sess, uint32_t n, uint32_t lds_cells,
                                         uint32_t max_groups, hipStream_t stream) {
  if (n == 0) return 0;
  lzgpu_host::LaunchShape s;
  if (!lzgpu_session_launch_shape(n, lds_cells, max_groups, 0, nullptr, &s)) return -1;
  auto kfn = s.win_bytes ? lzgpu_session_coop_kernel<true> : lzgpu_session_coop_kernel<false>;
  if (s.lds_bytes > 64 * 1024 && allow_full_lds(reinterpret_cast<const void*>(kfn)) != 0)
    return -1;
  hipLaunchKernelGGL(kfn, dim3(s.grid), dim3(s.block), s.lds_bytes, stream, d_sess, n, lds_cells,
                     s.win_bytes);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzgpu_launch_decode_batch(const LzmaGpuStreamDesc* d_descs, const uint32_t* d_order,
                                         uint32_t n, const uint8_t* d_src, uint8_t* d_dst,
                                         uint16_t* d_ws, LzmaGpuResult* d_results,
                                         hipStream_t stream) {
  if (n == 0) return 0;
  const uint32_t block = 64;
  const uint32_t grid = (n + block - 1) / block;
  hipLaunchKernelGGL(lzgpu_decode_batch_kernel, dim3(grid), dim3(block), 0, stream, d_descs,
                     d_order, n, d_src, d_dst, d_ws, d_results);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Every build of the three LDS decode kernels, by what decode_launch_shape
// names it with: family, W, placement, K2.  The kernels of a family share one
// signature whatever their template arguments.
struct KernelRow {
  uint32_t family, w, mask, k2;
  const void* fn;
};
#define LZ_ROWS_W(F, K, W, M)                                      \
  {F, W, M, 0u, reinterpret_cast<const void*>(K<W, M, false>)},    \
      {F, W, M, 1u, reinterpret_cast<const void*>(K<W, M, true>)},
#define LZ_ROWS_W24(F, K, M) LZ_ROWS_W(F, K, 2, M) LZ_ROWS_W(F, K, 4, M)
#define LZ_ROWS_W124(F, K, M) LZ_ROWS_W(F, K, 1, M) LZ_ROWS_W24(F, K, M)
static const KernelRow kDecodeKernels[] = {
    LZ_ROWS_W124(lzgpu_host::kFamLds, lzgpu_decode_lds_kernel, LZGPU_LDS_MASK)
    LZ_ROWS_W124(lzgpu_host::kFamLds, lzgpu_decode_lds_kernel, LZGPU_LDS_MASK | kIlvBit)
    LZ_ROWS_W124(lzgpu_host::kFamLds, lzgpu_decode_lds_kernel, LZGPU_LDS_MASK_LAT)
    LZ_ROWS_W124(lzgpu_host::kFamDup, lzgpu_decode_dup_kernel, LZGPU_LDS_MASK_LAT)
    LZ_ROWS_W124(lzgpu_host::kFamDup, lzgpu_decode_dup_kernel, kLdsMaskLatSlotG)
    // one wave per workgroup: W = 1 would not raise the register budget
    LZ_ROWS_W24(lzgpu_host::kFamCoop, lzgpu_decode_coop_kernel, LZGPU_LDS_MASK_LAT | kCoopBit)
    LZ_ROWS_W24(lzgpu_host::kFamCoop, lzgpu_decode_coop_kernel, LZGPU_LDS_MASK_ALL | kCoopBit)
    LZ_ROWS_W24(lzgpu_host::kFamCoop, lzgpu_decode_coop_kernel,
                LZGPU_LDS_MASK_ALL | kCoopBit | kWinBit)};
#undef LZ_ROWS_W124
#undef LZ_ROWS_W24
#undef LZ_ROWS_W

using LdsKernel = decltype(&lzgpu_decode_lds_kernel<1, LZGPU_LDS_MASK, false>);
using DupKernel = decltype(&lzgpu_decode_dup_kernel<1, LZGPU_LDS_MASK_LAT, false>);
using CoopKernel = decltype(&lzgpu_decode_coop_kernel<2, LZGPU_LDS_MASK_LAT | kCoopBit, false>);

extern "C" uint32_t lzgpu_decode_kernel_rows(uint32_t* rows, uint32_t cap) {
  uint32_t k = 0;
  for (const KernelRow& r : kDecodeKernels) {
    if (k < cap) memcpy(rows + 4 * k, &r, 4 * sizeof(uint32_t));  // family, w, mask, k2
    ++k;
  }
  return k;
}

extern "C" int lzgpu_decode_launch_shape(const LzmaGpuLdsClass* c, uint32_t n, uint32_t max_groups,
                                         uint32_t cus, const lzgpu_host::LaunchEnv* env,
                                         lzgpu_host::LaunchShape* out) {
  return lzgpu_host::decode_launch_shape(*c, n, max_groups, cus ? cus : lzgpu_host::device_cus(),
                                         env ? *env : launch_env(), *out);
}

extern "C" int lzgpu_launch_decode_lds(const LzmaGpuLdsClass& c, const LzgpuDecodeBufs& b,
                                       uint32_t max_groups, hipStream_t stream) {
  const uint32_t n = uint32_t(c.n);
  if (n == 0) return 0;
  lzgpu_host::LaunchShape s;
  if (!lzgpu_decode_launch_shape(&c, n, max_groups, 0, nullptr, &s)) return -1;
  const void* fn = nullptr;
  for (const KernelRow& r : kDecodeKernels)
    if (r.family == s.family && r.w == s.w && r.mask == s.mask && r.k2 == s.k2) fn = r.fn;
  if (!fn) return -1;  // no kernel built for this placement
  if (allow_full_lds(fn) != 0) return -1;
  if (hipMemsetAsync(b.queue, 0, sizeof(uint32_t), stream) != hipSuccess) return -1;
  const dim3 grid(s.grid), block(s.block);
  const uint32_t stride = c.lds_cells_per_lane;
  if (s.family == lzgpu_host::kFamLds)
    hipLaunchKernelGGL(LdsKernel(fn), grid, block, s.lds_bytes, stream, b.descs, b.order, n, b.src,
                       b.dst, b.ws, b.results, stride, b.queue, c.slot_off, c.slot_cells,
                       s.lanes_total);
  else if (s.family == lzgpu_host::kFamDup)
    hipLaunchKernelGGL(DupKernel(fn), grid, block, s.lds_bytes, stream, b.descs, b.order, n, b.src,
                       b.dst, b.ws, b.results, stride, b.queue);
  else
    hipLaunchKernelGGL(CoopKernel(fn), grid, block, s.lds_bytes, stream, b.descs, b.order, n,
                       b.src, b.dst, b.ws, b.results, stride, b.queue, s.win_bytes);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int lzgpu_launch_session(LzgpuSession* d_sess, uint32_t n, hipStream_t stream) {
  if (n == 0) return 0;
  const uint32_t block = 64;
  const uint32_t grid = (n + block - 1) / block;
  hipLaunchKernelGGL(lzgpu_session_kernel, dim3(grid), dim3(block), 0, stream, d_sess, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

#if LZGPU_PROF
// profiling builds: read (and optionally clear) the region cycle sums -- 40
// counters, out[22] = the build's LZGPU_PROF level
extern "C" int LzmaGpu_ProfileRead(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(lzgpu::g_lz_prof), 40 * sizeof(unsigned long long)) !=
      hipSuccess)
    return -1;
  out[22] = LZGPU_PROF;
  if (reset) {
    unsigned long long z[40] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(lzgpu::g_lz_prof), z, sizeof z) != hipSuccess) return -1;
  }
  return 0;
}
#endif
