// launch_plan_check.cpp -- csrc/launch_plan.h as a stand-alone host program
// (tests/test_launch_plan.py builds it with g++ -Wall -Werror and the address
// and undefined-behaviour sanitizers).  Input, one case per line:
//   limit n work_0 slice_0 ... work_{n-1} slice_{n-1}
// Output, one line per case: "over" when one slice alone exceeds the limit
// (and the plan came back empty), else
//   ok ws_max | order... | ws_off... | cut...
#include <inttypes.h>
#include <stdio.h>

#include <vector>

#include "launch_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  uint64_t limit, n;
  while (fscanf(f, "%" SCNu64 " %" SCNu64, &limit, &n) == 2) {
    // exact-size arrays: a read past either end is the sanitizer's to report
    std::vector<uint64_t> work(n), slice(n);
    for (uint64_t i = 0; i < n; ++i)
      if (fscanf(f, "%" SCNu64 " %" SCNu64, &work[i], &slice[i]) != 2) return 2;
    lzgpu_host::LaunchPlan p;
    p.ws_max = 77;  // whatever a plan held before is gone on failure
    p.cut.assign(3, 5);
    const bool ok = lzgpu_host::launch_plan(
        size_t(n), [&](uint32_t i) { return work.at(i); }, [&](uint32_t i) { return slice.at(i); },
        limit, p);
    if (!ok) {
      if (!p.order.empty() || !p.ws_off.empty() || !p.cut.empty() || p.ws_max != 0) return 3;
      printf("over\n");
      continue;
    }
    printf("ok %" PRIu64 " |", p.ws_max);
    for (uint32_t v : p.order) printf(" %u", v);
    printf(" |");
    for (uint64_t v : p.ws_off) printf(" %" PRIu64, v);
    printf(" |");
    for (size_t v : p.cut) printf(" %zu", v);
    printf("\n");
  }
  fclose(f);
  return 0;
}
