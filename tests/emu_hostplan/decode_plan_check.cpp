// decode_plan_check.cpp -- csrc/decode_plan.h as a stand-alone host program
// (tests/test_decode_plan.py builds it with g++ -Wall -Werror, -DLZGPU_HOST_EMU
// and the address and undefined-behaviour sanitizers): plans a batch and
// resolves the launch shape of every class of the plan, as on a device of the
// case's CUs with the default environment (32 lanes per one-stream wave,
// windows on).  Input, one case per line:
//   n cus kernel lanes groups waves persistent coop one_class flags npat tail
//   then npat + tail items "kind props_size b0 b1 b2 b3 b4"
// Item i of the batch is pattern item i mod npat, the last one the tail item if
// there is one; src_len, dst_off and dst_cap by the formula of
// tests/decode_plan_cases.py.  Output, one line per case:
//   res | the plan's 50 fields | crc32(probs_off[]) crc32(order[]) | shape; ...
// with a shape "family w mask k2 grid block win_bytes lanes_total lds_bytes",
// or "none" where no kernel is built for the class.
#include <inttypes.h>
#include <stdio.h>

#include <vector>

#include "decode_plan.h"

static uint32_t crc32(const void* data, size_t n) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int j = 0; j < 8; ++j) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
  }
  return c ^ 0xFFFFFFFFu;
}

static bool read_item(FILE* f, LzmaGpuStreamDesc& d) {
  unsigned kind, size, b[5];
  if (fscanf(f, "%u %u %u %u %u %u %u", &kind, &size, &b[0], &b[1], &b[2], &b[3], &b[4]) != 7)
    return false;
  d = LzmaGpuStreamDesc();
  for (int k = 0; k < 5; ++k) d.props[k] = uint8_t(b[k]);
  d.props_size = uint8_t(size);
  d.finish_mode = 1;
  d.kind = uint8_t(kind);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  uint64_t n;
  while (fscanf(f, "%" SCNu64, &n) == 1) {
    LzmaGpuPlanOptions o = LzmaGpuPlanOptions();
    unsigned npat, tail;
    if (fscanf(f, "%u %u %u %u %u %u %u %u %u %u %u", &o.cus, &o.kernel, &o.lanes_per_group,
               &o.groups_per_cu, &o.waves_per_simd, &o.persistent, &o.coop, &o.one_class, &o.flags,
               &npat, &tail) != 11 ||
        npat == 0)
      return 2;
    std::vector<LzmaGpuStreamDesc> pat(npat + tail);
    for (LzmaGpuStreamDesc& d : pat)
      if (!read_item(f, d)) return 2;
    // exact-size arrays: a read or write past either end is the sanitizer's to report
    std::vector<LzmaGpuStreamDesc> descs(n);
    for (uint64_t i = 0; i < n; ++i) {
      descs[i] = tail && i == n - 1 ? pat[npat] : pat[i % npat];
      descs[i].src_len = 100 + 10 * (37 * i % 97);
      descs[i].dst_off = 4096 * i;
      descs[i].dst_cap = 256 * (1 + i % 5);
    }
    std::vector<uint32_t> order(n ? n : 1);  // never null: the planner refuses a null order
    LzmaGpuPlan p;
    const SRes res = lzgpu_host::plan_batch(descs.data(), size_t(n), order.data(), &p, o, o.cus);
    printf("%d |", int(res));
    printf(" %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %u %u %" PRIu64 " %u %u", p.workspace_bytes,
           p.n, p.n_lds, p.lanes_per_group, p.lds_cells_per_lane, p.groups_per_cu,
           p.waves_per_simd, p.queue_offset, p.persistent, p.n_classes);
    for (const LzmaGpuLdsClass& c : p.classes)
      printf(" %" PRIu64 " %u %u %u %u %u %u %" PRIu64 " %u %u", c.n, c.lanes_per_group,
             c.lds_cells_per_lane, c.groups_per_cu, c.waves_per_simd, c.lds_mask, c.flags,
             c.slot_off, c.slot_cells, c.slot_groups);
    std::vector<uint64_t> probs(n);
    for (uint64_t i = 0; i < n; ++i) probs[i] = descs[i].probs_off;
    printf(" | %u %u |", crc32(probs.data(), 8 * probs.size()), crc32(order.data(), 4 * n));
    const lzgpu_host::LaunchEnv env{32, 0};
    for (uint32_t k = 0; k < p.n_classes; ++k) {
      const LzmaGpuLdsClass& c = p.classes[k];
      const uint32_t max_groups = p.persistent ? o.cus * c.groups_per_cu : 0u;
      lzgpu_host::LaunchShape s;
      if (lzgpu_host::decode_launch_shape(c, uint32_t(c.n), max_groups, o.cus, env, s))
        printf(" %u %u %u %u %u %u %u %u %" PRIu64 ";", s.family, s.w, s.mask, s.k2, s.grid,
               s.block, s.win_bytes, s.lanes_total, s.lds_bytes);
      else
        printf(" none;");
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
