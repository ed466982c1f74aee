// TEST INFRASTRUCTURE ONLY: host build of the SHA-256 kernels' per-lane and
// per-wave code (tests/test_sha256.py loads it with ctypes).
#include "sha_emu.h"

extern "C" {

void emu_sha256_lane(const uint8_t* p, uint64_t len, const uint32_t* init, uint64_t prior,
                     int finalise, uint8_t* out) {
  sha_emu::lane(p, len, init, prior, finalise, out);
}

void emu_sha256_wave(const uint8_t* p, uint64_t len, const uint32_t* init, uint64_t prior,
                     int finalise, uint8_t* out) {
  sha_emu::wave(p, len, init, prior, finalise, out);
}

uint32_t emu_sha256_super_bytes(void) { return lzgpu::kSha256Super * lzgpu::kSha256Block; }
}
