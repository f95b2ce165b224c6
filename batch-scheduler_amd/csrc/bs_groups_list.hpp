// bs_groups_list.hpp — group-list surgery on the device (bs_groups_list_apply): PodGroups enter and leave the cache (controller.go:194-196,
// :143, :167, :305) and the resident group pack, the queue's group column, the bound-pod table's and the wait table's follow in place.
// tu_groups.hip alone emits the kernels (a unity build includes it).
//
// Kernels, handed over by launch boundary only (every value written in one launch is read in a later one); plain vector loads and
// stores, one atomic add per pod whose group left; no kernel waits for another block:
//   k_gl_gather<S>  one thread per OLD group and one per appended group: the one pass over the group pack.  An old group i searches the
//                   sorted remove list once: lo = the removed indices below i; map[i] = -1 when i itself is listed, else i - lo, its new
//                   index.  A survivor's row goes to map[i] of the NEW pack — from the delta's rows when the sorted update list names i
//                   (all eight columns are replaced), else from the old pack as the device holds it.  Appended group k goes to
//                   g_old - n_remove + k from row n_update + k of the delta's rows.  Every new row is written exactly once.  The
//                   MinResources lanes are indexed by unrolled constants only (L = 4 + S).
//   k_gl_remap      one thread per entry of an int32 group column (the queue's, the bound table's, the wait table's survivors'): a value
//                   in 0 .. g_old - 1 becomes map[value]; -1 there is BS_POD_GROUP_MISSING and counts in the column's count word.  The
//                   sentinels and values at or above g_old stay as they are.
#pragma once

#include "bs_common.hpp"

namespace bs {

// the eight columns of a group pack; minres is [L][stride]
struct GlPack {
  uint32_t* min_member;
  uint32_t* status_scheduled;
  uint32_t* matched;
  uint8_t* flags;
  uint32_t* cls;
  int64_t* minres;
  uint32_t* mrpres;
  uint64_t* occupied;
  uint32_t stride;
};

struct GlDev {
  GlPack src, dst, rows;                // the old pack [g_old], the new pack [g_new], the delta's rows [n_update + n_append]
  uint32_t g_old, g_new;
  const uint32_t* rem;                  // [n_remove] OLD indices, ascending, distinct
  const uint32_t* upd;                  // [n_update] OLD indices, ascending, distinct
  uint32_t n_remove, n_update, n_append;
  int32_t* map;                         // [g_old] new index, -1 for a removed group
};

// entries of the ascending list below `key`
__device__ __forceinline__ uint32_t gl_below(const uint32_t* list, uint32_t count, uint32_t key) {
  uint32_t lo = 0, hi = count;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (list[mid] < key) lo = mid + 1u;
    else hi = mid;
  }
  return lo;
}

template <int S>
__global__ __launch_bounds__(256) void k_gl_gather(GlDev a) {
  constexpr int L = 4 + S;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= a.g_old + a.n_append) return;
  bool delta = false;                                        // the row comes from the delta's rows, not from the old pack
  uint32_t s, d;
  if (t < a.g_old) {
    const uint32_t lo = gl_below(a.rem, a.n_remove, t);
    const bool gone = lo < a.n_remove && a.rem[lo] == t;
    a.map[t] = gone ? -1 : (int32_t)(t - lo);
    if (gone) return;
    d = t - lo;
    s = t;
    const uint32_t u = gl_below(a.upd, a.n_update, t);
    if (u < a.n_update && a.upd[u] == t) { delta = true; s = u; }
  } else {
    const uint32_t k = t - a.g_old;
    d = a.g_old - a.n_remove + k;
    s = a.n_update + k;
    delta = true;
  }
  const uint32_t fstride = delta ? a.rows.stride : a.src.stride;
  if (d >= a.g_new || d >= a.dst.stride || s >= fstride) return;
  // (the columns are picked one by one: a pointer to a pack inside the kernel arguments would send them through private memory)
  a.dst.min_member[d] = (delta ? a.rows.min_member : a.src.min_member)[s];
  a.dst.status_scheduled[d] = (delta ? a.rows.status_scheduled : a.src.status_scheduled)[s];
  a.dst.matched[d] = (delta ? a.rows.matched : a.src.matched)[s];
  a.dst.flags[d] = (delta ? a.rows.flags : a.src.flags)[s];
  a.dst.cls[d] = (delta ? a.rows.cls : a.src.cls)[s];
  const int64_t* fmin = delta ? a.rows.minres : a.src.minres;
#pragma unroll
  for (int l = 0; l < L; ++l) a.dst.minres[(size_t)l * a.dst.stride + d] = fmin[(size_t)l * fstride + s];
  a.dst.mrpres[d] = (delta ? a.rows.mrpres : a.src.mrpres)[s];
  a.dst.occupied[d] = (delta ? a.rows.occupied : a.src.occupied)[s];
}

__global__ __launch_bounds__(256) void k_gl_remap(int32_t* col, uint32_t n, const int32_t* map, uint32_t g_old, uint32_t* missing) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int32_t v = col[i];
  if (v < 0 || (uint32_t)v >= g_old) return;
  const int32_t nv = map[v];
  if (nv == v) return;
  if (nv < 0) {
    col[i] = BS_POD_GROUP_MISSING;
    __hip_atomic_fetch_add(missing, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    col[i] = nv;
  }
}

}  // namespace bs
