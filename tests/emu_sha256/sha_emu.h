// TEST INFRASTRUCTURE ONLY: the two SHA-256 kernels of sha256_kernels.hip on
// the host, composed from sha256_device.h (LZGPU_HOST_EMU) the way the kernels
// compose it.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../lzma-sdk-zliblike_amd/csrc/sha256_device.h"

namespace sha_emu {

inline void start(const uint32_t* init, uint32_t st[8]) {
  if (init)
    memcpy(st, init, 32);
  else
    lzgpu::sha256_iv(st);
}

// lzgpu_sha256_lane_kernel, one lane
inline void lane(const uint8_t* p, uint64_t len, const uint32_t* init, uint64_t prior,
                 int finalise, uint8_t* out) {
  uint32_t st[8];
  start(init, st);
  lzgpu::sha256_lane(p, len, prior, finalise != 0, st);
  lzgpu::sha256_st_words(out, st, finalise != 0);
}

// lzgpu_sha256_wave_kernel, one wave: the lanes' halves run one after another
// where the device runs them side by side
inline void wave(const uint8_t* p, uint64_t len, const uint32_t* init, uint64_t prior,
                 int finalise, uint8_t* out) {
  using namespace lzgpu;
  static thread_local uint32_t park[64 * kSha256Super];  // [t][lane]
  uint32_t st[8];
  start(init, st);
  const uint64_t nb = sha256_num_blocks(len, finalise != 0), bits = (prior + len) << 3;
  uint32_t w[kSha256Super][16];
  for (uint32_t lane = 0; lane < kSha256Super; ++lane)
    if (lane < nb) sha256_message_block(p, len, bits, lane, w[lane]);
  for (uint64_t sb = 0; sb < nb; sb += kSha256Super) {
    const uint32_t cnt = nb - sb < kSha256Super ? uint32_t(nb - sb) : kSha256Super;
    for (uint32_t lane = 0; lane < cnt; ++lane)
      sha256_schedule(w[lane], [&](int t, uint32_t v) { park[t * kSha256Super + lane] = v; });
    for (uint32_t lane = 0; lane < kSha256Super; ++lane) {
      const uint64_t next = sb + kSha256Super + lane;
      if (next < nb) sha256_message_block(p, len, bits, next, w[lane]);
    }
    for (uint32_t j = 0; j < cnt; ++j)
      sha256_rounds(st, [&](int t) { return park[t * kSha256Super + j]; });
  }
  sha256_st_words(out, st, finalise != 0);
}

}  // namespace sha_emu
