// sevenzenc_internal.h -- the pack stage's launcher, shared by
// sevenzenc_kernels.hip and sevenzenc_capi.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lzma_gpu.h"

// The memset of the first-failed word and four launches on `stream` (collect,
// tiles, offsets, gather; with no pieces only tiles, which writes the total).
// 0 on success, -2 for more than 2^31 - 1 pieces, -1 if a launch failed.
extern "C" int szpackgpu_launch(const SzGpuPackArgs* args, hipStream_t stream);
