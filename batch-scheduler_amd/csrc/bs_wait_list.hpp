// bs_wait_list.hpp — the host-side checks of the bs_wait_* arguments (plain C++, no HIP: tests/native/wait_list_main.cpp compiles it
// alone).  Everything the calls refuse with BS_ERR_INVALID is found here, before anything is launched, except the one thing only the table
// knows: whether an id bs_wait_forget names is still live (k_wt_scan2, bs_wait.hpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bs {

constexpr uint32_t kWaitExpireDeny = 1u;   // BS_SEQ_EXPIRE_DENY: the one flag bs_wait_expire knows

enum WaitListError : int {
  kWlOk = 0,
  kWlFlags = 1,   // a flag bit other than BS_SEQ_EXPIRE_DENY
  kWlNull = 2,    // a NULL list with a count above 0
  kWlRange = 3,   // a group index >= g, an id >= the id space
  kWlTwice = 4,   // a group or an id listed twice
  kWlNode = 5,    // bs_wait_load: a node >= n
  kWlGroup = 6,   // bs_wait_load: a group outside 0 .. g - 1
};

inline const char* wait_list_text(int e) {
  switch (e) {
    case kWlOk: return "ok";
    case kWlFlags: return "unknown flag bits (BS_SEQ_EXPIRE_DENY is the only one)";
    case kWlNull: return "a list is NULL with a count above 0";
    case kWlRange: return "a group index or an id is out of range";
    case kWlTwice: return "a group or an id is listed twice";
    case kWlNode: return "an entry's node is not below the node count";
    case kWlGroup: return "an entry's group is not in 0 .. g - 1";
  }
  return "invalid";
}

inline int wait_flags_check(uint32_t flags) { return (flags & ~kWaitExpireDeny) ? kWlFlags : kWlOk; }

// A list of distinct values below `bound` (groups: the loaded group count; ids: the table's id space).  The list is not changed.
inline int wait_list_check(uint32_t bound, uint32_t count, const uint32_t* list) {
  if (!count) return kWlOk;
  if (!list) return kWlNull;
  if (count > bound) {                                      // more entries than values: bound + 1 of them in range repeat one — answered from
    for (uint32_t i = 0; i <= bound; ++i)                   // the first bound + 1 entries, nothing of the list's size is read or allocated
      if (list[i] >= bound) return kWlRange;
    return kWlTwice;
  }
  for (uint32_t i = 0; i < count; ++i)
    if (list[i] >= bound) return kWlRange;
  std::vector<uint32_t> seen(list, list + count);
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return kWlTwice;
  return kWlOk;
}

// bs_wait_load's columns as a whole: every node below n, every group in 0 .. g - 1
inline int wait_load_check(uint32_t n, uint32_t g, uint32_t w, const uint32_t* node, const int32_t* group) {
  if (!w) return kWlOk;
  if (!node || !group) return kWlNull;
  for (uint32_t i = 0; i < w; ++i) {
    if (node[i] >= n) return kWlNode;
    if (group[i] < 0 || (uint32_t)group[i] >= g) return kWlGroup;
  }
  return kWlOk;
}

}  // namespace bs
