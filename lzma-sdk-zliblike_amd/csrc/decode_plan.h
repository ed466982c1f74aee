// decode_plan.h -- the batch decoder's planner (plan_batch: placement, lanes,
// workgroups per CU and register budget of each class; behind the LzmaGpu_Plan*
// entry points) and launch shape (decode_launch_shape / session_launch_shape:
// kernel build, grid, block and LDS bytes; behind lzma_kernels.hip's launchers).
// Host arithmetic only -- no HIP include of its own, no HIP call, the CU count an
// argument: tests/emu_hostplan/ builds it with g++ -DLZGPU_HOST_EMU.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/lzma_gpu.h"
#include "lzma_device.h"

namespace lzgpu_host {

// LDS is given to a workgroup in whole blocks: 128 blocks of 1,280 bytes make a
// CU's 160 KiB (measured, profiles/r05_cfg5groups/: a launch padded to 160 KiB
// / 15 = 10,752 bytes per workgroup fitted 14 per CU, not 15 -- 9 blocks
// each).  Workgroup counts and the LDS padding that forces them are computed in
// blocks.
constexpr uint32_t kLdsBytesPerCu = 160u * 1024u;
constexpr uint32_t kLdsGrain = 1280u;
constexpr uint32_t kLdsBlocksPerCu = kLdsBytesPerCu / kLdsGrain;
inline uint32_t lds_blocks(size_t bytes) {
  return uint32_t((bytes + kLdsGrain - 1) / kLdsGrain);
}
// workgroups of `bytes` of LDS that fit a CU at once
inline uint32_t lds_groups_fit(size_t bytes) {
  const uint32_t b = lds_blocks(bytes);
  return b ? kLdsBlocksPerCu / b : 0xFFFFu;
}
// the most LDS each of `groups` workgroups can take with all of them resident
inline size_t lds_share(uint32_t groups) {
  return size_t(kLdsBlocksPerCu / (groups ? groups : 1u)) * kLdsGrain;
}

// ------------------------------------------------------------------ planner

// LDS cells of item d's slice under placement mask m (LZGPU_LDS_MASK_ALL: its
// whole table); 0 = bad props
inline uint32_t item_cells(const LzmaGpuStreamDesc& d, uint32_t m) {
  uint32_t lc = 4, lp = 0, pb = 4, dict;  // LZMA2 ranges: the lc+lp=4, pb=4 maximum
  if (d.kind == LZMA_GPU_KIND_LZMA2 ? d.props[0] > 40
                                    : lzgpu::lz_props_parse(d.props, d.props_size, lc, lp, pb,
                                                            dict) != lzgpu::kOk)
    return 0;
  return lzgpu::make_layout(lc, lp, pb, m).lds_cells;
}

// Workspace: each item gets a 16-byte aligned slice of table_cells() cells (an
// LZMA2 range whatever its prop byte: the kernel refuses a bad one by its own
// per-stream code).  Returns the bytes.
// `skip` (optional): items whose global sections live in a class slot area
// (lane-interleaved throughput classes) get no slice (probs_off 0, unused).
inline uint64_t plan_workspace(LzmaGpuStreamDesc* descs, size_t n,
                               const std::vector<uint8_t>* skip = nullptr) {
  uint64_t off = 0;
  for (size_t i = 0; i < n; ++i) {
    LzmaGpuStreamDesc& d = descs[i];
    if (skip && (*skip)[i]) {
      d.probs_off = 0;
      continue;
    }
    const uint32_t np = d.kind == LZMA_GPU_KIND_LZMA2 ? lzgpu::table_cells(4, 0, 4)
                                                      : item_cells(d, LZGPU_LDS_MASK_ALL);
    d.probs_off = off;
    off += (uint64_t(np) + 7) & ~uint64_t(7);
  }
  return off * 2;
}

// LzmaGpu_PlanBatch: slices, and streams of equal capacity and table width
// side by side
inline size_t plan_simple(LzmaGpuStreamDesc* descs, size_t n, uint32_t* order) {
  const uint64_t bytes = plan_workspace(descs, n);
  if (order) {
    std::vector<uint32_t> w(n);
    for (size_t i = 0; i < n; ++i) {
      w[i] = item_cells(descs[i], LZGPU_LDS_MASK);
      order[i] = uint32_t(i);
    }
    std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) {
      if (descs[a].dst_cap != descs[b].dst_cap) return descs[a].dst_cap > descs[b].dst_cap;
      return w[a] > w[b];
    });
  }
  return size_t(bytes);
}

// Launch shape of one LDS class: `stride` cells per stream, `count` streams,
// `cus` CUs.  `regime`: 0 = by the batch (throughput when LDS holds >= 64
// streams per CU and the batch fills them), 1 = throughput shape forced,
// 2 = latency shape (one stream per wave) forced.
inline LzmaGpuLdsClass plan_lds_class(uint32_t stride, uint64_t count, uint32_t mask, uint32_t cus,
                                      int regime, const LzmaGpuPlanOptions& o,
                                      bool* latency = nullptr, bool allow_fit = false) {
  LzmaGpuLdsClass c;
  memset(&c, 0, sizeof c);
  c.lds_mask = mask;
  // Per-lane slice: an odd number of dwords, so that the 32 lanes of a wave
  // reading the same cell index (literal-tree top levels, IsRep of one state)
  // fall in 32 different LDS banks (bank = dword mod 32 for 2- and 4-byte
  // reads); 8-byte aligned slices (158 dwords at lc0/pb0) put lanes l and
  // l + 16 in one bank.  Cells are read 2 or 4 bytes at a time: 4-byte
  // aligned slices suffice.
  if (o.flags & LZMA_GPU_PLAN_SLICE_ALIGN8)
    stride = (stride + 3) & ~3u;
  else
    stride = ((stride + 1) & ~1u) | 2u;  // cells = 2 mod 4: odd dword count
  const uint32_t per_cu = std::max<uint32_t>(1, kLdsBytesPerCu / (stride * 2));  // streams/CU
  uint32_t occ = 4;
  const uint32_t occ_over = o.waves_per_simd;
  if (occ_over == 1 || occ_over == 2 || occ_over == 4 || occ_over == 6 || occ_over == 8)
    occ = occ_over;
  // Two regimes (profiles/r01_variants v17-v28):
  //  * throughput -- LDS holds >= 64 streams per CU and the batch fills them:
  //    up to 32 streams per wave with at least 8 waves per CU (64K x 4 KiB:
  //    32 lanes x 8 waves per CU).  A VALU instruction of a wave whose active
  //    lanes all sit in its low half costs one pass whether 16 or 32 lanes are
  //    active, so 32 lanes halve the instructions per stream (ubench:
  //    scripts/ubench/lit_ubench.hip; v38-v41: 24.6 -> 27.0 GB/s with the
  //    checkpoint reader);
  //  * latency -- few streams per CU (small batches, or wide lc+lp tables):
  //    one stream per wave, 16 waves per CU (config 2: 5.8 GB/s vs 2.5 GB/s
  //    with 4 lanes x 4 waves; config 5: 2.6 GB/s vs 2.2 GB/s with 2 lanes).
  // Throughput shapes keep lanes and workgroups per CU powers of two; every
  // count is checked in LDS blocks below (lds_groups_fit).
  auto pow2floor = [](uint32_t v) {
    while (v & (v - 1)) v &= v - 1;
    return v;
  };
  const uint64_t per_cu_batch = (count + cus - 1) / cus;
  const bool thr = regime == 1 || (regime == 0 && per_cu >= 64 && per_cu_batch >= 64);
  uint32_t lanes = 1, groups = 16;
  if (latency) *latency = !thr;
  if (thr) {
    lanes = std::max<uint32_t>(1, std::min<uint32_t>(32, pow2floor(std::max<uint32_t>(1, per_cu / 8))));
    groups = pow2floor(std::max<uint32_t>(1, std::min<uint32_t>(per_cu / lanes, 16)));
  } else {
    // one lane per wave: as many waves as LDS allows -- counted in the CU's
    // 1,280-byte LDS blocks (lds_groups_fit) -- up to the 16 the register
    // budget keeps resident.  Round 1's "a power of two, 6 / 10 / 12 per CU
    // run 10-30 % slower" was this count taken in bytes: the padded slices of
    // 6, 10, 12 or 15 workgroups do not all fit, the last one waits for the
    // queue to drain (config 5: 15 planned, 14 resident, 5.6 GB/s; 14 planned
    // 7.2, profiles/r05_cfg5groups/)
    groups = std::min<uint32_t>(lds_groups_fit(size_t(stride) * 2), 16);
    // Fitted latency shape (strong-scaling shares, profiles/r03_shares/): a
    // batch of 17-63 streams per CU would run one-stream waves in two or more
    // rounds; widen the waves instead so that every stream is resident at
    // once -- 8,192 x 4 KiB (32 per CU): 2 lanes x 16 waves 5.64 ms vs 7.46 ms
    // in two rounds (and vs 5.95 ms for 4-lane throughput waves).  Only for a
    // batch that is one class (mixed-width batches merge their one-lane
    // classes instead: config 5 4.58 GB/s fitted vs 5.00).
    // LZMA_GPU_PLAN_NO_THR_FIT: the round-2 shape.
    if (allow_fit && !(o.flags & LZMA_GPU_PLAN_NO_THR_FIT) && regime != 2 &&
        per_cu_batch > groups && per_cu_batch < 64 && groups > 0) {
      uint32_t want = uint32_t((per_cu_batch + groups - 1) / groups);
      uint32_t l = 1;
      while (l < want) l <<= 1;
      while (l > 1 && uint64_t(l) * groups > per_cu) l >>= 1;
      lanes = l;
    }
  }
  const uint32_t over = o.lanes_per_group;
  if (over > 0 && over <= 64 && over * stride * 2 <= kLdsBytesPerCu) {
    lanes = over;
    groups = pow2floor(std::max<uint32_t>(1, std::min<uint32_t>(per_cu / lanes, 16)));
  }
  if (occ_over) groups = std::min<uint32_t>(groups, 4 * occ);
  // every planned workgroup resident at once, in whole LDS blocks
  const uint32_t fit = lds_groups_fit(size_t(lanes) * stride * 2);
  while (groups > 1 && groups > fit) groups = lanes == 1 ? groups - 1 : pow2floor(groups - 1);
  const uint32_t g_over = o.groups_per_cu;
  if (g_over > 0 && g_over <= fit) groups = g_over;
  c.n = count;
  c.lanes_per_group = lanes;
  c.lds_cells_per_lane = stride;
  c.groups_per_cu = std::max<uint32_t>(1, groups);
  // register budget = the waves per SIMD that are actually resident (one
  // wave per workgroup): 8 workgroups per CU -> 2 waves/SIMD -> 256 VGPRs,
  // enough for the decoder state without spills
  c.waves_per_simd = occ_over ? occ : std::max<uint32_t>(1, (c.groups_per_cu + 3) / 4);
  return c;
}

// LDS class of a stream by its table width (cells): narrow tables share a
// launch with many streams per CU, wide ones (lc + lp >= 3) get their own.
inline int lds_bucket(uint32_t cells) {
  return cells <= 768 ? 0 : cells <= 1536 ? 1 : cells <= 3072 ? 2 : 3;
}

// LzmaGpu_PlanBatchEx / Opt for `cus` CUs (the entry points pass o.cus, else
// the device's).  May throw std::bad_alloc.
inline SRes plan_batch(LzmaGpuStreamDesc* descs, size_t n, uint32_t* order, LzmaGpuPlan* plan,
                       const LzmaGpuPlanOptions& o, uint32_t cus) {
  if (!order || !plan) return SZ_ERROR_PARAM;
  if (o.kernel > LZMA_GPU_KERNEL_GLOBAL) return SZ_ERROR_PARAM;
  memset(plan, 0, sizeof *plan);
  plan->workspace_bytes = plan_workspace(descs, n);
  plan->n = n;
  // widest slice of the streams `idx` under placement mask m
  auto widest = [&](const std::vector<uint32_t>& idx, uint32_t m) {
    uint32_t s = 0;
    for (uint32_t i : idx) s = std::max(s, item_cells(descs[i], m));
    return s;
  };
  // LDS-eligible: lo table <= 16384 cells (32 KiB, >= 5 streams per CU)
  const uint32_t kMaxLdsCells = 16384;
  const bool global_only = o.kernel == LZMA_GPU_KERNEL_GLOBAL;
  const bool one_class = o.one_class != 0;
  std::vector<uint32_t> w(n), bucket_idx[LZMA_GPU_MAX_CLASSES], glob_idx;
  uint32_t bucket_stride[LZMA_GPU_MAX_CLASSES] = {0, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    w[i] = item_cells(descs[i], LZGPU_LDS_MASK);
    if (!global_only && w[i] != 0 && w[i] <= kMaxLdsCells) {
      const int b = one_class ? 0 : lds_bucket(w[i]);
      bucket_idx[b].push_back(uint32_t(i));
      bucket_stride[b] = std::max(bucket_stride[b], w[i]);
    } else {
      glob_idx.push_back(uint32_t(i));
    }
  }
  // Longest work first, and streams of similar work side by side: a wave
  // runs until its slowest lane is done.  Work ~ range-coder decisions, which
  // track the compressed bits (~1.5 decisions per input bit on text), plus a
  // little per output byte for literals writes and match copies.
  auto work = [&](uint32_t i) { return 24 * descs[i].src_len + descs[i].dst_cap; };
  auto by_len = [&](uint32_t a, uint32_t b) {
    const uint64_t wa = work(a), wb = work(b);
    if (wa != wb) return wa > wb;
    return w[a] > w[b];
  };
  // One class per width bucket: the throughput placement first; a class that
  // lands in the latency regime is re-planned with the latency placement (more
  // tables in LDS, few streams per CU); few streams per CU go cooperative.
  // The cooperative kernel is for few streams per CU -- counted over every
  // LDS-eligible stream of the batch, since the classes run side by side and
  // share the CUs (round 6: config 5's 4,096-stream share -- 16 per CU -- was
  // four classes of ~4 per CU, each planned cooperative with the whole CU's
  // LDS to itself and then starved of it when launched together: 246 ms,
  // against 132 ms for 16,384 streams of the same mix)
  size_t lds_total = 0;
  for (int b = 0; b < LZMA_GPU_MAX_CLASSES; ++b) lds_total += bucket_idx[b].size();
  const uint64_t per_cu_lds = (lds_total + cus - 1) / cus;
  auto plan_bucket = [&](const std::vector<uint32_t>& idx, uint32_t stride_lo,
                         bool allow_fit) -> LzmaGpuLdsClass {
    bool lat = false;
    const int regime = o.kernel == LZMA_GPU_KERNEL_THROUGHPUT ? 1 : 0;
    LzmaGpuLdsClass c = plan_lds_class(stride_lo, idx.size(), LZGPU_LDS_MASK, cus, regime, o, &lat);
    const bool want_lat = o.kernel == LZMA_GPU_KERNEL_LATENCY || o.kernel == LZMA_GPU_KERNEL_COOP ||
                          (o.kernel == LZMA_GPU_KERNEL_AUTO && lat);
    if (!want_lat) return c;
    const uint32_t stride_lat = widest(idx, LZGPU_LDS_MASK_LAT);
    if (stride_lat > kMaxLdsCells) return c;
    const int regime_lat = o.kernel == LZMA_GPU_KERNEL_AUTO ? 0 : 2;
    c = plan_lds_class(stride_lat, idx.size(), LZGPU_LDS_MASK_LAT, cus, regime_lat, o, nullptr,
                       allow_fit);
    // few streams per CU: the wave-cooperative kernel (all 32 lanes on one
    // stream, copies and direct bits spread over the lanes) -- config 4
    // 1.71 -> 2.85 GB/s and the xz leg 1.45 -> 2.36 at 4 streams per CU;
    // at 16 per CU (config 2) the single-lane waves are faster (5.9 vs 5.2)
    const uint64_t per_cu_batch = (idx.size() + cus - 1) / cus;
    const bool coop = o.kernel == LZMA_GPU_KERNEL_COOP ||
                      (o.kernel == LZMA_GPU_KERNEL_AUTO &&
                       (o.coop == 1 || (o.coop == 0 && per_cu_lds <= 8)));
    if (c.lanes_per_group == 1 && coop) {
      c.lds_mask = LZGPU_LDS_MASK_LAT | lzgpu::kCoopBit;
      if (!(o.flags & LZMA_GPU_PLAN_COOP_LAT)) {
        // the whole table in LDS if it still fits the streams per CU the
        // latency plan gives this class: no global round trip left in the
        // match path (SpecPos, LenHigh) or the matched literal
        const uint32_t stride_all = widest(idx, LZGPU_LDS_MASK_ALL);
        if (stride_all != 0 && stride_all <= kMaxLdsCells) {
          LzmaGpuLdsClass ca = plan_lds_class(stride_all, idx.size(),
                                              LZGPU_LDS_MASK_ALL | lzgpu::kCoopBit, cus, 2, o);
          const uint64_t want = std::min<uint64_t>(per_cu_batch, c.groups_per_cu);
          if (ca.lanes_per_group == 1 && ca.groups_per_cu >= want) c = ca;
        }
      }
    }
    // more streams per CU than the widest slice lets resident: the slot trees
    // to the global rows where that fits more one-stream workgroups per CU
    // (config 5: 14 -> 16)
    if (c.lds_mask == LZGPU_LDS_MASK_LAT && c.lanes_per_group == 1 && c.groups_per_cu < 16 &&
        per_cu_batch > c.groups_per_cu && !(o.flags & LZMA_GPU_PLAN_NO_SLOTG)) {
      const uint32_t stride_sg = widest(idx, lzgpu::kLdsMaskLatSlotG);
      if (stride_sg != 0 && stride_sg <= kMaxLdsCells) {
        const LzmaGpuLdsClass cs =
            plan_lds_class(stride_sg, idx.size(), lzgpu::kLdsMaskLatSlotG, cus, regime_lat, o);
        if (cs.lanes_per_group == 1 && cs.groups_per_cu > c.groups_per_cu) c = cs;
      }
    }
    return c;
  };
  // Several buckets in the one-lane latency regime (mixed-props batches,
  // config 5) become one class: its lanes draw from one queue in one launch,
  // so the batch has one tail instead of one per class, and its workgroup
  // count per CU is what the widest slice allows (up to 16, any number: the
  // queue balances the SIMDs) -- config 5 4.6-4.8 -> 4.9 GB/s, and steadier
  // (profiles/r02_ab/cfg5_merge_lat_ab.log).  LZMA_GPU_PLAN_NO_MERGE_LAT keeps
  // one class per bucket.
  if (!one_class && !(o.flags & LZMA_GPU_PLAN_NO_MERGE_LAT)) {
    int lat_b[LZMA_GPU_MAX_CLASSES], n_lat = 0;
    for (int b = 0; b < LZMA_GPU_MAX_CLASSES; ++b) {
      if (bucket_idx[b].empty()) continue;
      const LzmaGpuLdsClass c = plan_bucket(bucket_idx[b], bucket_stride[b], false);
      if ((c.lds_mask == LZGPU_LDS_MASK_LAT || c.lds_mask == lzgpu::kLdsMaskLatSlotG) &&
          c.lanes_per_group == 1)
        lat_b[n_lat++] = b;
    }
    if (n_lat >= 2) {
      const int t = lat_b[0];
      for (int j = 1; j < n_lat; ++j) {
        const int b = lat_b[j];
        bucket_idx[t].insert(bucket_idx[t].end(), bucket_idx[b].begin(), bucket_idx[b].end());
        bucket_stride[t] = std::max(bucket_stride[t], bucket_stride[b]);
        bucket_idx[b].clear();
      }
    }
  }
  int n_buckets = 0;
  for (int b = 0; b < LZMA_GPU_MAX_CLASSES; ++b) n_buckets += bucket_idx[b].empty() ? 0 : 1;
  size_t k = 0;
  uint64_t best = 0;
  std::vector<uint8_t> in_slots;  // items of lane-interleaved classes
  uint64_t slot_total[LZMA_GPU_MAX_CLASSES] = {0, 0, 0, 0};
  for (int b = 0; b < LZMA_GPU_MAX_CLASSES; ++b) {
    if (bucket_idx[b].empty()) continue;
    std::stable_sort(bucket_idx[b].begin(), bucket_idx[b].end(), by_len);
    for (uint32_t i : bucket_idx[b]) order[k++] = i;
    LzmaGpuLdsClass c = plan_bucket(bucket_idx[b], bucket_stride[b], n_buckets == 1);
    if (o.flags & LZMA_GPU_PLAN_KERNEL_LZMA2) c.flags |= LZMA_GPU_CLASS_HAS_LZMA2;
    for (uint32_t i : bucket_idx[b])
      if (descs[i].kind == LZMA_GPU_KIND_LZMA2) {
        c.flags |= LZMA_GPU_CLASS_HAS_LZMA2;
        break;
      }
    const bool ilv_any = (o.flags & LZMA_GPU_PLAN_ILV_ANY) != 0;
    // interleaved LDS slices take whole 32-lane rows (decode_launch_shape): a
    // narrow workgroup of a wide table (2 lanes at lc + lp = 4: 32 x 8,676 bytes)
    // would ask for more LDS than a CU has, so it keeps its per-lane slices
    const size_t ilv_lds = size_t((c.lanes_per_group + lzgpu::kIlv - 1) / lzgpu::kIlv * lzgpu::kIlv) *
                           c.lds_cells_per_lane * 2;
    if (!(o.flags & LZMA_GPU_PLAN_NO_ILV) && c.lds_mask == LZGPU_LDS_MASK &&
        ilv_lds <= kLdsBytesPerCu &&
        (c.lanes_per_group == 32 || c.lanes_per_group == 64 || (ilv_any && c.lanes_per_group <= 64))) {
      // lane-interleaved global sections: one column per resident lane (the
      // lanes keep it across the streams they take from the queue); config 3
      // 28.1 -> 29.9 GB/s (profiles/r02_ilv/ilv_ab.log).  Only for whole lane
      // groups: a narrower workgroup would leave most of every row unused.
      uint32_t rows = 0;  // the widest global part: whole table less the LDS sections
      for (uint32_t i : bucket_idx[b])
        rows = std::max(rows, item_cells(descs[i], LZGPU_LDS_MASK_ALL) - w[i]);
      const uint64_t grid = (c.n + c.lanes_per_group - 1) / c.lanes_per_group;
      const uint64_t groups =
          o.persistent == 2 ? grid : std::min<uint64_t>(grid, uint64_t(cus) * c.groups_per_cu);
      const uint64_t lane_groups = (c.lanes_per_group + lzgpu::kIlv - 1) / lzgpu::kIlv;
      c.slot_cells = std::max<uint32_t>((rows + 1) & ~1u, 2);  // even: pairs of cells
      c.slot_groups = uint32_t(groups);
      slot_total[plan->n_classes] = groups * lane_groups * lzgpu::kIlv * c.slot_cells;
      c.lds_mask |= lzgpu::kIlvBit;
      if (in_slots.empty()) in_slots.assign(n, 0);
      for (uint32_t i : bucket_idx[b]) in_slots[i] = 1;
    }
    plan->classes[plan->n_classes++] = c;
    plan->n_lds += c.n;
    if (c.n > best) {
      best = c.n;
      plan->lanes_per_group = c.lanes_per_group;
      plan->lds_cells_per_lane = c.lds_cells_per_lane;
      plan->groups_per_cu = c.groups_per_cu;
      plan->waves_per_simd = c.waves_per_simd;
    }
  }
  std::stable_sort(glob_idx.begin(), glob_idx.end(), by_len);
  for (uint32_t i : glob_idx) order[k++] = i;
  plan->persistent = o.persistent == 2 ? 0u : 1u;
  // per-stream slices only for items outside the slot areas, then the slot
  // areas (128-byte aligned), then the LDS launches' work counters
  uint64_t ws_cells = plan->workspace_bytes / 2;
  if (!in_slots.empty()) ws_cells = plan_workspace(descs, n, &in_slots) / 2;
  for (uint32_t c = 0; c < plan->n_classes; ++c) {
    if (!slot_total[c]) continue;
    ws_cells = (ws_cells + 63) & ~uint64_t(63);
    plan->classes[c].slot_off = ws_cells;
    ws_cells += slot_total[c];
  }
  plan->workspace_bytes = ws_cells * 2;
  plan->queue_offset = (plan->workspace_bytes + 63) & ~uint64_t(63);
  plan->workspace_bytes = plan->queue_offset + 64 * LZMA_GPU_MAX_CLASSES;
  return SZ_OK;
}

// ------------------------------------------------------------------ launch shape

// The launchers' two environment switches, read once per process
// (lzma_kernels.hip): LZGPU_DUP=D lanes of a one-stream wave (default 32; D = 1
// launches the one-lane kernel), LZGPU_WIN=0 no LDS history window.
struct LaunchEnv {
  int32_t dup;
  uint32_t win_off;
};
enum : uint32_t { kFamLds = 0, kFamDup = 1, kFamCoop = 2 };
// What a class launches with.  (family, w, mask, k2) is a row of lzma_kernels.hip's
// table: w = the W of __launch_bounds__, k2 = the build with the LZMA2 chunk walker,
// mask = the placement, with kWinBit when a window of win_bytes follows the table.
struct LaunchShape {
  uint32_t family, w, mask, k2;
  uint32_t grid, block;
  uint32_t win_bytes;
  uint32_t lanes_total;  // streams started before the first queue ticket
  uint64_t lds_bytes;    // dynamic LDS per workgroup
};

// Window for a launch of `grid` one-wave workgroups whose tables take
// `table_bytes` of LDS: the largest power of two that still leaves room for
// every workgroup a CU holds at once (one each while the grid fits the CUs),
// at most 128 KiB; 0 (no window) below 4 KiB.
inline uint32_t window_bytes(uint64_t grid, size_t table_bytes, uint32_t groups_per_cu,
                             uint32_t cus) {
  uint64_t per_cu = (grid + cus - 1) / cus;
  if (groups_per_cu && per_cu > groups_per_cu) per_cu = groups_per_cu;
  if (per_cu == 0) per_cu = 1;
  const size_t share = lds_share(uint32_t(per_cu));
  const size_t tb = (table_bytes + 15) & ~size_t(15);
  if (share <= tb + 4096) return 0;
  uint32_t w = 1u << 17;
  while (w > share - tb) w >>= 1;
  return w >= 4096 ? w : 0;
}

// Workgroups a CU actually holds at once: the launch's workgroups spread over
// the CUs, so at most min(groups_per_cu, ceil(n / cus)).  The register budget
// (the W of __launch_bounds__) follows it: a plan for 16 narrow-table
// cooperative waves per CU that gets one stream (a lone drop-in call) would
// otherwise run the W = 4 build, 128 VGPRs and 46-218 spilled, instead of the
// W = 2 build without spills.
inline uint32_t resident_waves_per_simd(uint32_t n, uint32_t groups_per_cu, uint32_t cus) {
  const uint32_t per_cu = std::max(1u, std::min(groups_per_cu, (n + cus - 1) / cus));
  return (per_cu + 3) / 4;
}

// workgroups of a launch under the cap of the persistent plans (0 = no cap)
inline uint32_t capped(uint32_t grid, uint32_t max_groups) {
  return max_groups && grid > max_groups ? max_groups : grid;
}

// s.grid cooperative workgroups, one stream each at a time: the table (s.lds_bytes),
// then the window where `win_mask` (the windowed build's placement, 0 = none built)
// and the launch leave room for one, else the table padded to the workgroup's share.
inline void coop_shape(LaunchShape& s, uint32_t groups_per_cu, uint32_t win_mask, uint32_t cus,
                       const LaunchEnv& env) {
  const uint64_t table = s.lds_bytes;
  s.family = kFamCoop;
  s.block = 32;
  s.lanes_total = s.grid;
  if (win_mask && !env.win_off) s.win_bytes = window_bytes(s.grid, table, groups_per_cu, cus);
  if (s.win_bytes) {
    s.mask = win_mask;
    s.lds_bytes = ((table + 15) & ~uint64_t(15)) + s.win_bytes;
  } else if (groups_per_cu) {
    s.lds_bytes = std::max<uint64_t>(table, lds_share(groups_per_cu));
  }
}

// Launch shape of n (> 0) streams of class c on a device of `cus` CUs, at most
// max_groups workgroups (0 = one launch round, no queue refills needed);
// false = no kernel is built for this class.
inline bool decode_launch_shape(const LzmaGpuLdsClass& c, uint32_t n, uint32_t max_groups,
                                uint32_t cus, const LaunchEnv& env, LaunchShape& s) {
  using namespace lzgpu;
  s = LaunchShape();
  const uint32_t lanes = c.lanes_per_group, groups_per_cu = c.groups_per_cu;
  if (n == 0 || lanes == 0) return false;
  cus = std::max(1u, cus);
  s.mask = c.lds_mask;
  s.k2 = (c.flags & LZMA_GPU_CLASS_HAS_LZMA2) ? 1u : 0u;
  s.lds_bytes = uint64_t(c.lds_cells_per_lane) * 2;
  // register budget: the class's, W = 4 for every plan above 2 (4, 6, 8) --
  // held to what is resident for one-stream workgroups only
  const uint32_t resident = resident_waves_per_simd(n, groups_per_cu, cus);
  auto build_w = [](uint32_t w) { return w <= 1 ? 1u : w == 2 ? 2u : 4u; };
  const bool dup_ok = env.dup > 1 && env.dup <= 64;
  const bool coop_all = c.lds_mask == (LZGPU_LDS_MASK_ALL | kCoopBit);
  if (coop_all || c.lds_mask == (LZGPU_LDS_MASK_LAT | kCoopBit)) {
    // one wave per workgroup: register budget by workgroups per SIMD; with the
    // whole table in LDS, the history window too where the launch has room
    s.w = resident <= 2 ? 2u : 4u;
    s.grid = capped(n, max_groups);
    coop_shape(s, groups_per_cu, coop_all ? c.lds_mask | kWinBit : 0u, cus, env);
    return true;
  }
  if (c.lds_mask == kLdsMaskLatSlotG) {
    // planned for one-stream workgroups only (plan_bucket)
    if (lanes != 1 || !dup_ok) return false;
    s.w = build_w(std::min(c.waves_per_simd, resident));
  } else if (c.lds_mask == LZGPU_LDS_MASK_LAT) {
    s.w = build_w(lanes == 1 ? std::min(c.waves_per_simd, resident) : c.waves_per_simd);
  } else if ((c.lds_mask & ~kIlvBit) == LZGPU_LDS_MASK) {
    s.w = build_w(c.waves_per_simd);
  } else {
    return false;
  }
  // pad each workgroup's LDS so that exactly groups_per_cu fit on a CU (an
  // even split over its four SIMDs), whatever the dispatcher would pack;
  // interleaved slices take whole 32-lane rows
  const bool ilv = (c.lds_mask & kIlvBit) != 0u;
  s.lds_bytes *= ilv && LZGPU_LDS_ILV != 0 ? (lanes + kIlv - 1) / kIlv * kIlv : lanes;
  if (groups_per_cu) s.lds_bytes = std::max<uint64_t>(s.lds_bytes, lds_share(groups_per_cu));
  s.grid = capped((n + lanes - 1) / lanes, max_groups);
  if (ilv) {
    // the slot area holds slot_groups workgroups' columns; persistent lanes
    // cover the rest of the batch from the queue
    if (c.slot_groups == 0 || lanes > 64) return false;
    if (s.grid > c.slot_groups) {
      if (!max_groups) return false;
      s.grid = c.slot_groups;
    }
  }
  s.lanes_total = s.grid * lanes;
  // one-stream waves of the latency placements: env.dup lanes on the stream
  const bool dup = !ilv && c.lds_mask != LZGPU_LDS_MASK && lanes == 1 && dup_ok;
  s.family = dup ? kFamDup : kFamLds;
  s.block = dup ? uint32_t(env.dup) : lanes;
  return true;
}

// Launch shape of n (> 0) cooperative sessions with tables of at most lds_cells
// cells (lzgpu_session_coop_kernel; w and k2 do not apply): the window is sized with
// no cap on the workgroups per CU.  false = the table does not fit a CU's LDS.
inline bool session_launch_shape(uint32_t n, uint32_t lds_cells, uint32_t max_groups, uint32_t cus,
                                 const LaunchEnv& env, LaunchShape& s) {
  s = LaunchShape();
  if (n == 0 || lds_cells == 0 || size_t(lds_cells) * 2 > kLdsBytesPerCu) return false;
  s.mask = LZGPU_LDS_MASK_ALL | lzgpu::kCoopBit;
  s.lds_bytes = uint64_t(lds_cells) * 2;
  s.grid = capped(n, max_groups);
  coop_shape(s, 0, s.mask | lzgpu::kWinBit, std::max(1u, cus), env);
  return true;
}

}  // namespace lzgpu_host
