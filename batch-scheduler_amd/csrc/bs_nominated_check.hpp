// bs_nominated_check.hpp — what the bs_nominated_* calls and BS_PREEMPT_NOMINATE refuse on the host before anything is launched: the NULL
// rules, a snapshot's nodes against the node count, the remove list against the live ids (the context keeps them, ascending: the table is
// small), the insert list against the queue length and the node count, and the row count and the id space against their limits.
// Nothing is left for the device to find: a call that passes these checks cannot fail there.
// Plain C++17, no HIP header: tests/test_nominated_cpu.py compiles it alone under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace bs {

constexpr uint32_t kNomMaxRows = 1u << 16;   // BS_NOM_MAX
constexpr uint32_t kNomMaxIds = 1u << 24;    // the id space between two loads

enum : int {
  kNomOk = 0,
  kNomNull = 1,       // a required array is NULL with a count above 0                    (BS_ERR_INVALID)
  kNomNode = 2,       // a node index at or above the node count                           (BS_ERR_INVALID)
  kNomIdUnknown = 3,  // a remove id at or above the id space                               (BS_ERR_INVALID)
  kNomIdDead = 4,     // a remove id that is not in the table (removed earlier)            (BS_ERR_INVALID)
  kNomIdTwice = 5,    // a remove id listed twice                                          (BS_ERR_INVALID)
  kNomPodIndex = 6,   // a pod index at or above the queue length                          (BS_ERR_INVALID)
  kNomRows = 7,       // more than BS_NOM_MAX live rows afterwards                         (BS_ERR_CAPACITY)
  kNomIdSpace = 8,    // the id space would pass 2^24                                      (BS_ERR_CAPACITY)
};
inline bool nom_check_is_capacity(int code) { return code == kNomRows || code == kNomIdSpace; }

// bs_nominated_load: m rows on n nodes.  The row limit is judged first: a snapshot that is too large is not walked.
inline int nom_load_check(uint32_t n, uint32_t m, const uint32_t* node, const int32_t* priority, const int64_t* req, const uint32_t* req_present,
                          uint32_t max_rows = kNomMaxRows) {
  if (m > max_rows) return kNomRows;
  if (m && (!node || !priority || !req || !req_present)) return kNomNull;
  for (uint32_t i = 0; i < m; ++i)
    if (node[i] >= n) return kNomNode;
  return kNomOk;
}

// bs_nominated_apply.  live[w]: the table's ids, ascending; ids: the id space; p: the queue length; n: the node count.
inline int nom_apply_check(const uint32_t* live, uint32_t w, uint32_t ids, uint32_t n_remove, const uint32_t* remove_id, uint32_t n_insert,
                           const uint32_t* pod_index, const uint32_t* node, const int32_t* priority, uint32_t p, uint32_t n,
                           uint32_t max_rows = kNomMaxRows, uint32_t max_ids = kNomMaxIds) {
  if (n_remove && !remove_id) return kNomNull;
  if (n_insert && (!pod_index || !node || !priority)) return kNomNull;
  for (uint32_t r = 0; r < n_remove; ++r)
    if (remove_id[r] >= ids) return kNomIdUnknown;
  if (n_remove) {
    std::vector<uint32_t> seen(remove_id, remove_id + n_remove);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return kNomIdTwice;
    for (uint32_t id : seen)
      if (!w || !std::binary_search(live, live + w, id)) return kNomIdDead;
  }
  for (uint32_t k = 0; k < n_insert; ++k) {
    if (pod_index[k] >= p) return kNomPodIndex;
    if (node[k] >= n) return kNomNode;
  }
  // (the remove list is distinct and live here: n_remove <= w.)  Sums in 64 bits: n_insert may be near 2^32.
  if ((uint64_t)w - n_remove + n_insert > (uint64_t)max_rows) return kNomRows;
  if ((uint64_t)ids + n_insert > (uint64_t)max_ids) return kNomIdSpace;
  return kNomOk;
}

// BS_PREEMPT_NOMINATE: judged against `count`, the most rows the call can append, before its first launch
inline int nom_nominate_check(uint32_t w, uint32_t ids, uint32_t count, uint32_t max_rows = kNomMaxRows, uint32_t max_ids = kNomMaxIds) {
  if ((uint64_t)w + count > (uint64_t)max_rows) return kNomRows;
  if ((uint64_t)ids + count > (uint64_t)max_ids) return kNomIdSpace;
  return kNomOk;
}

// bs_seq_run_nominated: own_id[p] (NULL: nobody has a row) names, per queue pod, the row that IS the pod, or `none`.  Every id that is
// not `none` must be live and named by one pod only (kNomIdUnknown / kNomIdDead / kNomIdTwice).  own_row[p] = the row's index in the table
// (live[] is the table's order), `none` where the pod has no row; left untouched on a refusal.
inline int nom_own_check(const uint32_t* live, uint32_t w, uint32_t ids, uint32_t p, const uint32_t* own_id, uint32_t none, std::vector<uint32_t>& own_row) {
  std::vector<uint32_t> rows(p, none);
  if (own_id) {
    std::vector<uint8_t> named(w, 0);
    for (uint32_t i = 0; i < p; ++i) {
      const uint32_t id = own_id[i];
      if (id == none) continue;
      if (id >= ids) return kNomIdUnknown;
      const uint32_t* at = std::lower_bound(live, live + w, id);
      if (at == live + w || *at != id) return kNomIdDead;
      const uint32_t r = (uint32_t)(at - live);
      if (named[r]) return kNomIdTwice;
      named[r] = 1;
      rows[i] = r;
    }
  }
  own_row.swap(rows);
  return kNomOk;
}
inline const char* nom_own_check_text(int code) {
  switch (code) {
    case kNomIdUnknown: return "an own id is at or above bs_nominated_ids";
    case kNomIdDead: return "an own id is not in the table (removed, cleared or consumed earlier)";
    case kNomIdTwice: return "an own id is named by two pods";
  }
  return "ok";
}

inline const char* nom_check_text(int code) {
  switch (code) {
    case kNomOk: return "ok";
    case kNomNull: return "a required array is NULL with a count above 0";
    case kNomNode: return "a node index is at or above the node count";
    case kNomIdUnknown: return "a remove id is at or above bs_nominated_ids";
    case kNomIdDead: return "a remove id is not in the table (removed earlier)";
    case kNomIdTwice: return "a remove id is listed twice";
    case kNomPodIndex: return "a pod index is at or above the queue length";
    case kNomRows: return "more than BS_NOM_MAX rows";
    case kNomIdSpace: return "the id space would pass 2^24: reload the table";
  }
  return "unknown";
}

}  // namespace bs
