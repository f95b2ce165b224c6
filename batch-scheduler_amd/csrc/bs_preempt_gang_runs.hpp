// bs_preempt_gang_runs.hpp — bs_preempt_commit_gang's runs (include/bsched.h), plain C++ for the host: from the slots' group indices in
// slot order and gang_need[g], the per-slot arrays k_gang_resolve reads (bs_preempt_commit.hpp, GangDev), and the rule that a group
// with a requirement forms exactly one run.  No HIP in here: tests/native/gang_runs_main.cpp compiles it alone.
#pragma once
#include <stdint.h>

#include <vector>

namespace bs {

// A run: a maximal sequence of consecutive slots whose pods share one group index grp >= 0 with gang_need[grp] > 0.
//   s_need[s]  the run's need for every slot of a run, 0 for a slot in no run
//   s_rlen[s]  the run's length where slot s ends a run, 0 elsewhere
// Returns the group index that forms a second run (the caller answers BS_ERR_INVALID), -1 when every group forms at most one.
// A group index >= g has no requirement (gang_need has g entries).
inline int32_t gang_runs(uint32_t q, const int32_t* sgroup, uint32_t g, const uint32_t* gang_need, std::vector<uint32_t>& s_need,
                         std::vector<uint32_t>& s_rlen) {
  s_need.assign(q, 0u);
  s_rlen.assign(q, 0u);
  std::vector<uint8_t> closed(g, 0);              // the group's run has ended
  auto need_of = [&](uint32_t s) -> uint32_t {
    const int32_t grp = sgroup[s];
    return grp >= 0 && (uint32_t)grp < g ? gang_need[grp] : 0u;
  };
  uint32_t s = 0;
  while (s < q) {
    const uint32_t need = need_of(s);
    if (!need) { ++s; continue; }
    const int32_t grp = sgroup[s];
    if (closed[grp]) return grp;
    uint32_t e = s;
    while (e + 1 < q && sgroup[e + 1] == grp) ++e;
    for (uint32_t i = s; i <= e; ++i) s_need[i] = need;
    s_rlen[e] = e - s + 1;
    closed[grp] = 1;
    s = e + 1;
  }
  return -1;
}

}  // namespace bs
