// bs_groups_list_check.hpp — the host side of bs_groups_list_apply (plain C++, no HIP: tests/native/groups_list_main.cpp compiles it
// alone).  Everything the call refuses with BS_ERR_INVALID is found here, before anything resident changes, and the index rule the
// device kernels follow (k_gl_gather, bs_groups_list.hpp) is stated once more in host terms: the largest group index the bound table is
// held to name moves by it.
#pragma once
#include <stdint.h>

namespace bs {

enum GroupsListError : int {
  kGlOk = 0,
  kGlNull = 1,    // a NULL array with a count or a capacity above 0
  kGlRows = 2,    // rows.g != n_update + n_append
  kGlRange = 3,   // a remove or update index at or above g
  kGlOrder = 4,   // a list that is not strictly ascending
};

inline const char* groups_list_text(int e) {
  switch (e) {
    case kGlOk: return "ok";
    case kGlNull: return "an array is NULL with a count or a capacity above 0";
    case kGlRows: return "rows.g is not n_update + n_append";
    case kGlRange: return "a remove or update index is not below the group count";
    case kGlOrder: return "a remove or update list is not strictly ascending";
  }
  return "invalid";
}

// one list of OLD indices: every entry below g, strictly ascending.  Entry by entry: the range first, then the order.
inline int groups_list_indices(uint32_t g, uint32_t count, const uint32_t* list) {
  for (uint32_t i = 0; i < count; ++i) {
    if (list[i] >= g) return kGlRange;
    if (i && list[i] <= list[i - 1]) return kGlOrder;
  }
  return kGlOk;
}

// The delta as a whole, in this order: the NULL arrays, the row count, the remove list, the update list.  rows_null: one of the eight
// columns of `rows` is NULL; wait_null: one of the three result arrays is.
inline int groups_list_check(uint32_t g, uint32_t n_remove, const uint32_t* remove, uint32_t n_update, const uint32_t* update, uint32_t rows_g,
                             bool rows_null, uint32_t n_append, uint32_t wait_cap, bool wait_null) {
  if ((n_remove && !remove) || (n_update && !update) || (rows_g && rows_null) || (wait_cap && wait_null)) return kGlNull;
  if ((uint64_t)rows_g != (uint64_t)n_update + n_append) return kGlRows;
  if (const int bad = groups_list_indices(g, n_remove, remove)) return bad;
  return groups_list_indices(g, n_update, update);
}

// entries of the ascending list below `key`
inline uint32_t groups_list_below(uint32_t count, const uint32_t* list, uint32_t key) {
  uint32_t lo = 0, hi = count;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (list[mid] < key) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

// The index rule: old group i becomes i minus the removed indices below it, -1 when i itself is removed (i < g).
inline int32_t groups_list_new_index(uint32_t i, uint32_t n_remove, const uint32_t* remove) {
  const uint32_t lo = groups_list_below(n_remove, remove, i);
  if (lo < n_remove && remove[lo] == i) return -1;
  return (int32_t)(i - lo);
}

// group count after the call
inline uint32_t groups_list_count(uint32_t g, uint32_t n_remove, uint32_t n_append) { return g - n_remove + n_append; }

// The largest group index a table is held to name (bs_ctx::bound_max_group), after the remap: a value at or above the old g, or below 0,
// stays; a surviving index moves with its group; a removed one falls to the largest new index a group below it can have (the map is
// monotone), which may be -1.
inline int32_t groups_list_max_group(int32_t m, uint32_t g, uint32_t n_remove, const uint32_t* remove) {
  if (m < 0 || (uint32_t)m >= g) return m;
  return (int32_t)((uint32_t)m - groups_list_below(n_remove, remove, (uint32_t)m + 1u));
}

}  // namespace bs
