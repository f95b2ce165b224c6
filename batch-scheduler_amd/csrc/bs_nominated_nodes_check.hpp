// bs_nominated_nodes_check.hpp — the host half of bs_nominated_nodes_apply (include/bsched.h): what the call refuses before anything
// resident changes, the delta list reduced to what the device needs (bs_bound_nodes_replay.hpp as it stands: the sorted OLD nodes that
// leave and the count the replay ends at), whether anything has to be launched at all, and the live ids after the dropped rows left.
// Plain C++17, no device header: tests/test_nominated_nodes_cpu.py compiles it alone under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <iterator>
#include <vector>

#include "bs_bound_nodes_replay.hpp"

namespace bs {

enum : int {
  kNomNodesOk = 0,
  kNomNodesNull = 1,     // n_out is NULL, kind or index is NULL with count > 0, a result array is NULL with cap > 0     (BS_ERR_INVALID)
  kNomNodesDelta = 2,    // a kind outside the three, an UPDATE / REMOVE index at or beyond the count at that point      (BS_ERR_INVALID)
  kNomNodesCount = 3,    // the replay ends at a count other than the node list's                                        (BS_ERR_STATE)
};
inline bool nom_nodes_check_is_state(int code) { return code == kNomNodesCount; }

// the NULL rules on their own: they are judged before the context's state
inline bool nom_nodes_null(uint32_t count, const uint32_t* kind, const uint32_t* index, uint32_t cap, const uint32_t* id, const uint32_t* node,
                           const int32_t* priority, const uint32_t* n_out) {
  return !n_out || (count && (!kind || !index)) || (cap && (!id || !node || !priority));
}

// n0: the node count the table was made for; n_now: bs_nodes_count.  On kNomNodesOk `out` holds the replay; nothing else is written.
inline int nom_nodes_check(uint32_t n0, uint32_t n_now, uint32_t count, const uint32_t* kind, const uint32_t* index, uint32_t cap, const uint32_t* id,
                           const uint32_t* node, const int32_t* priority, const uint32_t* n_out, NodeReplay& out) {
  if (nom_nodes_null(count, kind, index, cap, id, node, priority, n_out)) return kNomNodesNull;
  if (bound_nodes_replay(n0, count, kind, index, out)) return kNomNodesDelta;
  if (out.n_new != n_now) return kNomNodesCount;
  return kNomNodesOk;
}

// Rows move (and the heads are made again) unless the table is empty, or no old node leaves and the count stays: nhead's length is part
// of the table's layout, so a list that only grew needs heads for the new count although no row changes its node.
inline bool nom_nodes_moves(uint32_t w, uint32_t n0, const NodeReplay& rp) { return w != 0 && (!rp.removed.empty() || rp.n_new != n0); }

// live: the table's ids, ascending; gone[n]: the dropped ids, ascending (the device leaves them in table order).  Work: O(live).
inline void nom_nodes_live_drop(std::vector<uint32_t>& live, const uint32_t* gone, size_t n) {
  if (!n) return;
  std::vector<uint32_t> left;
  left.reserve(live.size() >= n ? live.size() - n : 0);
  std::set_difference(live.begin(), live.end(), gone, gone + n, std::back_inserter(left));
  live.swap(left);
}

inline const char* nom_nodes_check_text(int code) {
  switch (code) {
    case kNomNodesOk: return "ok";
    case kNomNodesNull: return "n_out is NULL, or an array is NULL with a count or capacity above 0";
    case kNomNodesDelta: return "a kind outside UPDATE / APPEND / REMOVE, or an index at or beyond the node count at its point of the replay";
    case kNomNodesCount: return "the replay does not end at the node count: not the list bs_nodes_apply got";
  }
  return "unknown";
}

}  // namespace bs
