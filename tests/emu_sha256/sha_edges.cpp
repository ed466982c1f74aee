// TEST INFRASTRUCTURE ONLY: over-read / over-write check of the SHA-256 device
// code on the host.  Built with -fsanitize=address,undefined and run as a
// program of its own (tests/test_sha256.py); never loaded into Python, never
// run on a GPU.
//
// Every range lives in a heap allocation of exactly a + len bytes and starts a
// bytes into it (a = 0..15: every start alignment, the allocator returning
// 16-byte aligned blocks), so the range's end is the allocation's end and at
// a = 0 its start is the allocation's start: a read one byte outside trips
// the sanitizer.  The 32 output bytes are an exact allocation too.  Both
// compositions (lane, wave) must agree, finalised and as a state continued in
// a second call.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sha_emu.h"

static int failures = 0;

static void one(uint64_t len, unsigned a) {
  uint8_t* buf = static_cast<uint8_t*>(malloc(a + len ? a + len : 1));
  uint8_t* p = buf + a;
  uint32_t x = uint32_t(len * 2654435761u + a * 40503u + 1);
  for (uint64_t i = 0; i < len; ++i) {
    x = x * 1664525u + 1013904223u;
    p[i] = uint8_t(x >> 24);
  }
  uint8_t* dl = static_cast<uint8_t*>(malloc(32));
  uint8_t* dw = static_cast<uint8_t*>(malloc(32));
  uint8_t* st = static_cast<uint8_t*>(malloc(32));
  uint8_t* d2 = static_cast<uint8_t*>(malloc(32));
  sha_emu::lane(p, len, nullptr, 0, 1, dl);
  sha_emu::wave(p, len, nullptr, 0, 1, dw);
  if (memcmp(dl, dw, 32) != 0) {
    fprintf(stderr, "lane != wave at len %llu align %u\n", (unsigned long long)len, a);
    ++failures;
  }
  // whole blocks first (state out), then the tail continued from that state
  const uint64_t whole = len & ~uint64_t(63);
  for (int k = 0; k < 2; ++k) {
    (k ? sha_emu::wave : sha_emu::lane)(p, len, nullptr, 0, 0, st);
    uint32_t init[8];
    memcpy(init, st, 32);
    // the tail in an exact allocation of its own
    uint8_t* tail = static_cast<uint8_t*>(malloc(len - whole ? len - whole : 1));
    memcpy(tail, p + whole, len - whole);
    (k ? sha_emu::lane : sha_emu::wave)(tail, len - whole, init, whole, 1, d2);
    free(tail);
    if (memcmp(dl, d2, 32) != 0) {
      fprintf(stderr, "continued != one-shot at len %llu align %u (%d)\n",
              (unsigned long long)len, a, k);
      ++failures;
    }
  }
  free(d2);
  free(st);
  free(dw);
  free(dl);
  free(buf);
}

int main() {
  const uint64_t S = uint64_t(lzgpu::kSha256Super) * lzgpu::kSha256Block;
  std::vector<uint64_t> lens;
  for (uint64_t l = 0; l <= 130; ++l) lens.push_back(l);
  for (uint64_t l : {S - 1, S, S + 1, S + 55, S + 56, S + 63, 2 * S - 1, 2 * S, 2 * S + 9})
    lens.push_back(l);
  for (uint64_t l : lens)
    for (unsigned a = 0; a < 16; ++a) one(l, a);
  printf("sha_edges: %zu lengths x 16 alignments, %d failures\n", lens.size(), failures);
  return failures ? 1 : 0;
}
