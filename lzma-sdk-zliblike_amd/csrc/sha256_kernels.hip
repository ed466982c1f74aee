// sha256_kernels.hip -- SHA-256 of byte ranges of device memory for gfx950
// (sha256_device.h; the xz SHA-256 block check and the Sha256.h drop-ins).
//
//   lzgpu_sha256_lane_kernel: one lane per range.  Issue-bound: the aggregate
//     rate grows with the lanes resident, so it is the kernel for many ranges.
//   lzgpu_sha256_wave_kernel: one wave per range, for few long ranges, where a
//     range is one serial chain and the aim is to shorten it.  Per pass the 64
//     lanes take 64 consecutive blocks (4 KiB, adjacent lanes adjacent blocks,
//     four 16-byte loads each), every lane computes its own block's schedule
//     W[t] + K[t] -- independent of the chaining state -- and parks it in LDS
//     as park[t][lane] (lane-contiguous rows: conflict-free stores, and the
//     rounds' reads are one broadcast address with t as the instruction's
//     offset).  The rounds of the 64 blocks then run in order with the state
//     wave-uniform, reading W + K from LDS off the dependency chain; the next
//     pass's global loads are issued before them.  The last partial pass and
//     the padding blocks go through the same path.
//
// Neither kernel touches a byte outside [off, off + len) of a range or outside
// its 32 output bytes.
#include <hip/hip_runtime.h>

#include "lzma_gpu_internal.h"
#include "sha256_device.h"

using namespace lzgpu;

namespace {

// a range's chaining state to start from and the bytes hashed before it
__device__ __forceinline__ void sha256_start(const uint32_t* __restrict__ init,
                                             const uint64_t* __restrict__ prior, uint32_t r,
                                             uint32_t st[8], uint64_t* before) {
  if (init) {
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = init[8 * size_t(r) + i];
  } else {
    sha256_iv(st);
  }
  *before = prior ? prior[r] : 0;
}

}  // namespace

__global__ void __launch_bounds__(64) lzgpu_sha256_lane_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
    const uint64_t* __restrict__ len, const uint32_t* __restrict__ init,
    const uint64_t* __restrict__ prior, uint32_t n, int finalise, uint8_t* __restrict__ out) {
  const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t st[8];
  uint64_t before;
  sha256_start(init, prior, uint32_t(i), st, &before);
  sha256_lane((const sha256_gbyte*)(data + off[i]), len[i], before, finalise != 0, st);
  sha256_st_words((sha256_gbyte*)(out + 32 * i), st, finalise != 0);
}

// 16 KiB of LDS per wave = 13 allocation blocks of 1,280 bytes: nine workgroups
// of one wave fit a CU's 160 KiB
__global__ void __launch_bounds__(64) lzgpu_sha256_wave_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ off,
    const uint64_t* __restrict__ len, const uint32_t* __restrict__ init,
    const uint64_t* __restrict__ prior, uint32_t n, int finalise, uint8_t* __restrict__ out) {
  __shared__ uint32_t park[64 * kSha256Super];  // [t][lane]
  const uint32_t lane = threadIdx.x;
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    const sha256_gbyte* p = (const sha256_gbyte*)(data + off[r]);
    const uint64_t size = len[r];
    uint32_t st[8];
    uint64_t before;
    sha256_start(init, prior, r, st, &before);
    const uint64_t nb = sha256_num_blocks(size, finalise != 0), bits = (before + size) << 3;
    uint32_t w[16];
    if (lane < nb) sha256_message_block(p, size, bits, lane, w);
    for (uint64_t sb = 0; sb < nb; sb += kSha256Super) {
      const uint32_t cnt = nb - sb < kSha256Super ? uint32_t(nb - sb) : kSha256Super;
      if (lane < cnt)
        sha256_schedule(w, [&](int t, uint32_t v) { park[t * kSha256Super + lane] = v; });
      __syncthreads();
      // the next pass's blocks, in flight during the rounds
      const uint64_t next = sb + kSha256Super + lane;
      if (next < nb) sha256_message_block(p, size, bits, next, w);
      // The state is wave-uniform, and left to itself the compiler splits the
      // rounds between the scalar and the vector unit (rotates on the vector
      // side, 448 v_readfirstlane per block to carry them back): measured
      // 79 ms per 1 MiB range against the lane kernel's 51 ms.  Pinned to vector
      // registers, the rounds stay on the vector unit.
#pragma unroll
      for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(st[i]));
      for (uint32_t j = 0; j < cnt; ++j)
        sha256_rounds(st, [&](int t) { return park[t * kSha256Super + j]; });
      __syncthreads();
    }
    if (lane == 0) sha256_st_words((sha256_gbyte*)(out + 32 * size_t(r)), st, finalise != 0);
  }
}

extern "C" int lzgpu_launch_sha256(const uint8_t* d_data, const uint64_t* d_off,
                                   const uint64_t* d_len, uint32_t n, const uint32_t* d_init,
                                   const uint64_t* d_prior, int finalise, unsigned kernel,
                                   uint8_t* d_out, hipStream_t stream) {
  if (n == 0) return 0;
  if (kernel == kLzgpuSha256Auto)
    kernel = n >= kLzgpuSha256AutoLaneMin ? kLzgpuSha256Lane : kLzgpuSha256Wave;
  if (kernel == kLzgpuSha256Lane) {
    hipLaunchKernelGGL(lzgpu_sha256_lane_kernel, dim3(n / 64 + (n % 64 != 0)), dim3(64), 0, stream, d_data,
                       d_off, d_len, d_init, d_prior, n, finalise, d_out);
  } else if (kernel == kLzgpuSha256Wave) {
    // every wave the chip holds at once (LDS: nine per CU), then a range stride
    const uint32_t fit = lzgpu_host::device_cus() *
                         lzgpu_host::lds_groups_fit(sizeof(uint32_t) * 64 * kSha256Super);
    hipLaunchKernelGGL(lzgpu_sha256_wave_kernel, dim3(n < fit ? n : fit), dim3(64), 0, stream,
                       d_data, d_off, d_len, d_init, d_prior, n, finalise, d_out);
  } else {
    return -2;
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
