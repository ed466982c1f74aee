// device_shim.h -- what lets the per-lane device headers compile twice: for
// gfx950, and as plain C++ under LZGPU_HOST_EMU (test-only host builds of the
// kernels' per-lane code, tests/emu*; never part of liblzmagpu.so).  The
// function qualifiers, and the aligned 16-byte global load the range
// primitives read with.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef LZGPU_HOST_EMU
#ifndef __device__
#define __device__
#define __host__
#define __forceinline__ inline
#endif
#else
#include <hip/hip_runtime.h>
#endif

namespace lzgpu {

#ifdef LZGPU_HOST_EMU
struct u32x4 {
  uint32_t x, y, z, w;
};
__device__ __forceinline__ u32x4 load16(uintptr_t a) {
  const uint32_t* p = (const uint32_t*)a;
  return u32x4{p[0], p[1], p[2], p[3]};
}
#else
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 load16(uintptr_t a) {
  return *(__attribute__((address_space(1))) const u32x4*)a;
}
#endif

}  // namespace lzgpu
