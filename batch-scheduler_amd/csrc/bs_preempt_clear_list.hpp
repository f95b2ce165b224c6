// bs_preempt_clear_list.hpp — the host's side of BS_PREEMPT_CLEAR_LOWER (include/bsched.h, rule C): the cleared rows as the context keeps
// them between the preemption call and bs_preempt_cleared_read, the check of what the device listed (k_nc_list) against the ids the
// context keeps before the list is handed to the table rewrite, and the read's NULL and cap rules.
// Plain C++17, no HIP header: tests/test_preempt_clear_cpu.py compiles it alone under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

namespace bs {

enum : int {
  kClrOk = 0,
  kClrNull = 1,     // n_out is NULL, or a column is NULL with cap above 0              (BS_ERR_INVALID)
  kClrState = 2,    // the last successful preemption call did not carry the flag       (BS_ERR_STATE)
  kClrCount = 3,    // the device listed more rows than the table holds                 (an internal error)
  kClrOrder = 4,    // the listed ids are not strictly ascending                        (an internal error)
  kClrDead = 5,     // a listed id is not live                                          (an internal error)
  kClrNode = 6,     // a listed node is at or above the node count, or `by` at or above the preemptor count
};

// the cleared rows of the last successful preemption call, ascending id
struct ClearedRows {
  std::vector<uint32_t> id, node, by;
  std::vector<int32_t> priority;
  bool have = false;          // that call carried BS_PREEMPT_CLEAR_LOWER
  void reset(bool flagged) {
    id.clear(); node.clear(); by.clear(); priority.clear();
    have = flagged;
  }
};

// What k_nc_list wrote, before anybody acts on it: count rows out of a table of w rows whose ids are live[w] (ascending), on n nodes, for
// q preemptors.  The list is a subsequence of the table, so it must be strictly ascending and every id live.
inline int clear_list_check(uint32_t count, const uint32_t* id, const uint32_t* node, const uint32_t* by, const uint32_t* live, uint32_t w, uint32_t n,
                            uint32_t q) {
  if (count > w) return kClrCount;
  if (count && (!id || !node || !by)) return kClrNull;
  for (uint32_t i = 0; i < count; ++i) {
    if (i && id[i] <= id[i - 1]) return kClrOrder;
    if (!w || !live || !std::binary_search(live, live + w, id[i])) return kClrDead;
    if (node[i] >= n || by[i] >= q) return kClrNode;
  }
  return kClrOk;
}

// bs_preempt_cleared_read behind its NULL ctx check: *n_out is the true count, the first min(n, cap) rows come back; the columns may be
// NULL when cap == 0 (and are not looked at when there is nothing to copy)
inline int clear_read(const ClearedRows& rows, uint32_t cap, uint32_t* id, uint32_t* node, int32_t* priority, uint32_t* by, uint32_t* n_out) {
  if (!n_out) return kClrNull;
  if (!rows.have) return kClrState;
  if (cap && (!id || !node || !priority || !by)) return kClrNull;
  const size_t n = rows.id.size(), k = std::min<size_t>(n, cap);
  if (k) {
    std::memcpy(id, rows.id.data(), k * 4);
    std::memcpy(node, rows.node.data(), k * 4);
    std::memcpy(priority, rows.priority.data(), k * 4);
    std::memcpy(by, rows.by.data(), k * 4);
  }
  *n_out = (uint32_t)n;
  return kClrOk;
}

inline const char* clear_check_text(int code) {
  switch (code) {
    case kClrOk: return "ok";
    case kClrNull: return "n_out is NULL, or a column is NULL with cap above 0";
    case kClrState: return "the last successful preemption call did not carry BS_PREEMPT_CLEAR_LOWER";
    case kClrCount: return "the device listed more cleared rows than the table holds";
    case kClrOrder: return "the cleared ids are not ascending";
    case kClrDead: return "a cleared id is not in the table";
    case kClrNode: return "a cleared row names a node or a preemptor that does not exist";
  }
  return "unknown";
}

}  // namespace bs
