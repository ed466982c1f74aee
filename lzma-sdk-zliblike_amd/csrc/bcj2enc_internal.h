// bcj2enc_internal.h -- the BCJ2 encoder's launcher (bcj2enc_kernels.hip), used
// by its C ABI and by the 7z writer's BCJ2 folders.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lzma_gpu.h"

// phases: the split (plan, classify, streams, scatter), the range coder, or
// both; the coder needs the split's scratch.  0 on success, -1 if a launch failed.
constexpr unsigned kBcj2EncSplit = 1, kBcj2EncCode = 2, kBcj2EncAll = 3;
extern "C" int bcj2encgpu_launch(const Bcj2GpuEncDesc* d_descs, uint32_t n, const uint8_t* d_src,
                                 uint8_t* d_dst, uint8_t* d_scratch, Bcj2GpuEncResult* d_results,
                                 unsigned phases, hipStream_t stream);
