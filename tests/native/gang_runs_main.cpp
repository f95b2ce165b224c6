// Stand-alone check of bs_preempt_gang_runs.hpp (tests/test_preempt_gang_cpu.py builds it with -fsanitize=address,undefined and runs it).
// Reads cases from stdin, one per line: "q g  group[0..q)  need[0..g)"; prints per case "bad" then need[0..q) then rlen[0..q).
#include <cstdio>
#include <vector>

#include "bs_preempt_gang_runs.hpp"

int main() {
  unsigned q, g;
  while (std::scanf("%u %u", &q, &g) == 2) {
    std::vector<int32_t> grp(q);
    std::vector<uint32_t> need(g), s_need, s_rlen;
    for (auto& v : grp) if (std::scanf("%d", &v) != 1) return 2;
    for (auto& v : need) if (std::scanf("%u", &v) != 1) return 2;
    const int32_t bad = bs::gang_runs(q, grp.data(), g, need.data(), s_need, s_rlen);
    std::printf("%d", bad);
    if (bad < 0) {
      for (uint32_t v : s_need) std::printf(" %u", v);
      for (uint32_t v : s_rlen) std::printf(" %u", v);
    }
    std::printf("\n");
  }
  return 0;
}
