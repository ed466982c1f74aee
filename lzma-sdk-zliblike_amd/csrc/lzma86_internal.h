// lzma86_internal.h -- the Lzma86 launchers, shared by lzma86_kernels.hip and
// lzma86_capi.hip.  Every launcher returns 0 on success.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lzma_gpu.h"
#include "lzma86_device.h"

// A chosen candidate of at most this many bytes is moved by the wave that made
// the choice; a longer one is split over the workgroups of a second launch,
// kLzma86PartBytes per workgroup.  LZGPU_LZMA86_SPLIT overrides the threshold
// for A/B runs (lzma86_bench.py).
constexpr uint64_t kLzma86SplitDefault = 32768;
constexpr uint64_t kLzma86PartBytes = 32768;
constexpr uint32_t kLzma86PartsMax = 1024;
uint64_t lzma86_split();

// the sources of the streams that get a filtered candidate, copied into the
// filter area; `parts` workgroups per job
extern "C" int lzma86gpu_launch_stage(const lz86::StageJob* d_jobs, uint32_t n, uint32_t parts,
                                      const uint8_t* src_base, uint8_t* filt_base,
                                      hipStream_t stream);
// choice, header and result of every stream and the move of the short ones;
// then the streams of d_large (those whose slot can hold more than `split`
// bytes) with `parts` workgroups each
extern "C" int lzma86gpu_launch_select(const lz86::Stream* d_streams, uint32_t n,
                                       const LzmaEncGpuResult* d_cand, const uint8_t* d_slots,
                                       uint8_t* d_dst, Lzma86GpuResult* d_results,
                                       const uint32_t* d_large, uint32_t n_large, uint32_t parts,
                                       uint64_t split, hipStream_t stream);
extern "C" int lzma86gpu_launch_finish(const lz86::DecStream* d_streams, uint32_t n,
                                       const LzmaGpuResult* d_lzma, Lzma86GpuResult* d_results,
                                       uint64_t* d_x86_len, hipStream_t stream);
