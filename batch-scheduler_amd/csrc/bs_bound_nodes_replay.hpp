// bs_bound_nodes_replay.hpp — the host half of bs_bound_nodes_apply (include/bsched.h): a bs_nodes_apply delta list, replayed on a node
// list of n0 nodes, reduced to what the bound table needs to follow it.  Plain C++ (no HIP): tests/test_bound_nodes_cpu.py compiles it on
// its own, with the sanitizers, against a Python restatement.
//
// During the replay the list is always [the surviving OLD nodes, in their old order] ++ [the surviving APPENDED nodes]: an append goes to
// the end and a remove keeps the order.  So a current index i names
//   i <  n0 - R   the i-th old node that is not removed yet (R = old nodes removed so far).  With the removed old indices sorted,
//                 r[0] < r[1] < ..., r[j] - j is the number of survivors in front of r[j] and does not fall with j: the old index is i + j
//                 for the first j with r[j] - j > i (j = R when there is none) — a binary search;
//   i >= n0 - R   an appended node.  Appended nodes hold no bound pods, so it does not matter WHICH one leaves: the remove cancels an append.
// Work: O(log count) comparisons per delta plus the insert into the sorted list (a memmove of at most R words) per remove of an old node.
#pragma once
#include <stdint.h>

#include <vector>

namespace bs {

constexpr uint32_t kNodeDeltaUpdate = 0u, kNodeDeltaAppend = 1u, kNodeDeltaRemove = 2u;   // BS_DELTA_* (include/bsched.h)

struct NodeReplay {
  std::vector<uint32_t> removed;   // OLD node indices that leave, ascending, distinct
  uint32_t appended = 0;           // appended nodes that are still there at the end
  uint32_t n_new = 0;              // n0 - removed.size() + appended
};

// 0 = fine; d + 1 = delta d is invalid (a kind outside the three, an UPDATE / REMOVE index at or beyond the count current at that point)
inline uint32_t bound_nodes_replay(uint32_t n0, uint32_t count, const uint32_t* kind, const uint32_t* index, NodeReplay& out) {
  std::vector<uint32_t>& r = out.removed;
  r.clear();
  uint32_t app = 0;
  for (uint32_t d = 0; d < count; ++d) {
    const uint32_t R = (uint32_t)r.size(), old_left = n0 - R, cur = old_left + app, i = index[d];
    if (kind[d] == kNodeDeltaAppend) {
      if (cur == UINT32_MAX) return d + 1u;
      ++app;
    } else if (kind[d] == kNodeDeltaUpdate) {
      if (i >= cur) return d + 1u;
    } else if (kind[d] == kNodeDeltaRemove) {
      if (i >= cur) return d + 1u;
      if (i >= old_left) { --app; continue; }
      uint32_t lo = 0, hi = R;                         // the first j with r[j] - j > i
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (r[mid] - mid <= i) lo = mid + 1u;
        else hi = mid;
      }
      r.insert(r.begin() + lo, i + lo);
    } else {
      return d + 1u;
    }
  }
  out.appended = app;
  out.n_new = n0 - (uint32_t)r.size() + app;
  return 0u;
}

}  // namespace bs
