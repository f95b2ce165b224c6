// bs_seq_expire_list.hpp — the host-side check of bs_seq_expire's arguments (plain C++, no HIP: tests/native/seq_expire_list_main.cpp
// compiles it alone).  Everything bs_seq_expire refuses with BS_ERR_INVALID is found here, before anything is launched.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bs {

constexpr uint32_t kSeqExpireDeny = 1u;   // BS_SEQ_EXPIRE_DENY
constexpr uint32_t kSeqExpireAll = 2u;    // BS_SEQ_EXPIRE_ALL

enum SeqExpireListError : int {
  kSeListOk = 0,
  kSeListFlags = 1,       // a flag bit the header does not define
  kSeListAllWithList = 2, // BS_SEQ_EXPIRE_ALL together with a list (group != NULL or count != 0)
  kSeListNull = 3,        // group == NULL without BS_SEQ_EXPIRE_ALL
  kSeListRange = 4,       // a group index >= g
  kSeListTwice = 5,       // a group listed twice
};

inline const char* seq_expire_list_text(int e) {
  switch (e) {
    case kSeListOk: return "ok";
    case kSeListFlags: return "bs_seq_expire: unknown flag bits";
    case kSeListAllWithList: return "bs_seq_expire: BS_SEQ_EXPIRE_ALL takes no list (group must be NULL and count 0)";
    case kSeListNull: return "bs_seq_expire: group is NULL without BS_SEQ_EXPIRE_ALL";
    case kSeListRange: return "bs_seq_expire: group index out of range";
    case kSeListTwice: return "bs_seq_expire: a group is listed twice";
  }
  return "bs_seq_expire: invalid";
}

// g = the loaded group count.  The list is not changed.
inline int seq_expire_list_check(uint32_t g, uint32_t count, const uint32_t* group, uint32_t flags) {
  if (flags & ~(kSeqExpireDeny | kSeqExpireAll)) return kSeListFlags;
  if (flags & kSeqExpireAll) return (group || count) ? kSeListAllWithList : kSeListOk;
  if (!group) return kSeListNull;
  if (count > g) {                                          // more entries than groups: g + 1 of them in range repeat one — answered from the
    for (uint32_t i = 0; i <= g; ++i)                       // first g + 1 entries, nothing of the list's size is read or allocated
      if (group[i] >= g) return kSeListRange;
    return kSeListTwice;
  }
  for (uint32_t i = 0; i < count; ++i)
    if (group[i] >= g) return kSeListRange;
  std::vector<uint32_t> seen(group, group + count);
  std::sort(seen.begin(), seen.end());
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return kSeListTwice;
  return kSeListOk;
}

}  // namespace bs
