// launch_plan.h -- how a host batch is laid out under a workspace limit: the
// streams longest first, cut into launches whose workspace slices fit the limit
// together.  Host arithmetic only (no HIP include): tests/emu_hostplan/ builds
// it with g++.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

namespace lzgpu_host {

struct LaunchPlan {
  std::vector<uint32_t> order;   // item order[k] is the k-th to start
  std::vector<uint64_t> ws_off;  // workspace offset of item order[k]
  std::vector<size_t> cut;       // launch c covers [cut[c], cut[c + 1]) of the order
  uint64_t ws_max = 0;           // the largest launch's workspace
};

// order[0..n): items 0..n-1 by descending work(i), ties in index order.  The
// waves or workgroups of a launch start in index order, so the longest start
// first.
template <class Work>
void longest_first(size_t n, Work work, uint32_t* order) {
  std::iota(order, order + n, 0u);
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t b) { return work(a) > work(b); });
}

// Walks the longest_first order: item order[k] takes slice(order[k]) bytes
// behind the launch's earlier items, and a new launch starts exactly when the
// slice would pass `limit` (non-zero).  An item with a slice of 0 -- a
// descriptor the kernel refuses with its own per-stream code -- still takes its
// place in the order and in a launch.  No launch is empty unless n == 0.
// false: one item's slice alone exceeds the limit; p is left empty.
template <class Work, class Slice>
bool launch_plan(size_t n, Work work, Slice slice, uint64_t limit, LaunchPlan& p) {
  p = LaunchPlan();
  std::vector<uint32_t> order(n);
  longest_first(n, work, order.data());
  std::vector<uint64_t> ws_off(n);
  std::vector<size_t> cut{0};
  uint64_t ws_max = 0, cur = 0;
  for (size_t k = 0; k < n; ++k) {
    const uint64_t need = slice(order[k]);
    if (need > limit) return false;
    if (cur + need > limit) {
      cut.push_back(k);
      cur = 0;
    }
    ws_off[k] = cur;
    cur += need;
    ws_max = std::max(ws_max, cur);
  }
  cut.push_back(n);
  p.order.swap(order);
  p.ws_off.swap(ws_off);
  p.cut.swap(cut);
  p.ws_max = ws_max;
  return true;
}

}  // namespace lzgpu_host
