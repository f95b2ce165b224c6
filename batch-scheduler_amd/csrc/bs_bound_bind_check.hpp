// bs_bound_bind_check.hpp — what bs_bound_bind refuses on the host before anything is launched: the NULL rules, the two lists against the
// wait table's id space and the queue length, and the bound table's id space against its limit.  Duplicates, dead ids and the pods' own
// state (no node, still waiting) are found on the device (bs_bound_bind.hpp, bs_wait.hpp) before anything resident is written.
// Plain C++17, no HIP header: tests/test_bound_bind_cpu.py compiles it alone under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bs {

enum : int {
  kBindOk = 0,
  kBindNull = 1,       // a required array is NULL with a count above 0
  kBindWaitId = 2,     // a wait id at or above the id space
  kBindWaitDead = 3,   // more wait ids than live rows: an id is dead or listed twice
  kBindPodIndex = 4,   // a pod index at or above the queue length
  kBindPodTwice = 5,   // more pod indices than the queue holds: one is listed twice
  kBindIdSpace = 6,    // the bound table's id space would pass its limit
};

// priority and start_ns are per row (wait rows first, then pods); pdb_violating, node_out and first_id_out may be NULL
inline int bind_args_check(uint32_t n_wait, const uint32_t* wait_id, uint32_t n_pod, const uint32_t* pod_index, const int32_t* priority,
                           const int64_t* start_ns) {
  if (n_wait && !wait_id) return kBindNull;
  if (n_pod && !pod_index) return kBindNull;
  if ((n_wait || n_pod) && (!priority || !start_ns)) return kBindNull;
  return kBindOk;
}

// wait_ids: the wait table's id space, wait_rows: its live rows; queue: the queue length
inline int bind_lists_check(uint32_t wait_ids, uint32_t wait_rows, uint32_t n_wait, const uint32_t* wait_id, uint32_t queue, uint32_t n_pod,
                            const uint32_t* pod_index) {
  for (uint32_t i = 0; i < n_wait; ++i)
    if (wait_id[i] >= wait_ids) return kBindWaitId;
  if (n_wait > wait_rows) return kBindWaitDead;
  for (uint32_t j = 0; j < n_pod; ++j)
    if (pod_index[j] >= queue) return kBindPodIndex;
  if (n_pod > queue) return kBindPodTwice;
  return kBindOk;
}

// ids: the bound table's id space; exactly `limit` is fine.  The sum is taken in 64 bits: both counts may be near 2^32.
inline int bind_ids_check(uint32_t ids, uint32_t n_wait, uint32_t n_pod, uint32_t limit) {
  return (uint64_t)ids + (uint64_t)n_wait + (uint64_t)n_pod > (uint64_t)limit ? kBindIdSpace : kBindOk;
}

inline const char* bind_check_text(int code) {
  switch (code) {
    case kBindOk: return "ok";
    case kBindNull: return "a required array is NULL with a count above 0";
    case kBindWaitId: return "a wait id is at or above bs_wait_ids";
    case kBindWaitDead: return "a wait id is not in the table, or is listed twice";
    case kBindPodIndex: return "a pod index is at or above the queue length";
    case kBindPodTwice: return "a pod index is listed twice";
    case kBindIdSpace: return "the id space would pass BS_BOUND_MAX: reload the table";
  }
  return "unknown";
}

}  // namespace bs
