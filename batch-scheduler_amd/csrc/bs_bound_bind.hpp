// bs_bound_bind.hpp — pods that leave Permit enter the bound table on the device (include/bsched.h, bs_bound_bind).  The rows come from two
// resident places: listed rows of the Permit-wait table (bs_wait.hpp: node, group, request lanes and present bits are columns) and listed
// pods of the queue the last pass placed (their node in the pass's result block, their lanes in the queue pack).  The kernels here build
// the insert block bs_bound_apply's host code builds — the rows sorted by (node, priority descending, start ascending, call order), ids
// ids + slot — and k_ba_scatter .. k_ba_merge (bs_bound_apply.hpp) run over it unchanged.  tu_bind.hip alone instantiates them.
//
// Launches, handed over by launch boundary only (plain loads and stores, atomics on the scratch words, vector stores only):
//   k_bb_rows<S>     one thread per wait row: a row the wait core marked (mark[id] = list position + 1, k_wt_mark) copies node / group /
//                    pres / req[L] to slot mark - 1.  One thread per listed pod: the index against the queue length, a claim in a zeroed
//                    bitmap over the queue (a second claim is the duplicate), pod_node >= 0, not in the pass's chains (wnode[], as k_wt_walk
//                    fills it) — a failed check goes into the error word; a pod that passes writes its node, its group as the queue stores
//                    it and its lanes by k_wt_gather's rule to slot n_wait + j.  Every written slot adds 1 to its node's count.
//   k_bb_scan1<S> /  the spread scan (k_wt_scan1 / k_wt_scan2's form over 32-bit counts): the exclusive scan of the per-node counts in blocks of
//   k_bb_scan2<S>    1024, the segment start of every node.
//   k_bb_scatter<S>  one thread per slot: into its node's segment through the node's cursor, in arbitrary order.
//   k_bb_rank<S>     one wave per node, four nodes per workgroup; a node without inserts returns at once.  The segment is ranked by counting,
//                    64 slots per step against 64-slot windows read by readlane (k_ba_merge's loop): slot i lands at segment start +
//                    #{j in the segment : j strictly before i in (priority desc, start asc, slot asc)}, which makes the order
//                    deterministic.  A segment longer than BS_BOUND_MAX_PER_NODE sets kBaErrFull in the patch's error word and is left.
//   k_bb_gather<S>   one thread per final position: the sorted block in BoundApplyDev's insert layout (inode, iprio, istart, igroup,
//                    ireq[L][I], iid = ids + slot, ipres, ipdb); priority, start and the PDB bit come from the host's blob by slot;
//                    node_out by slot; the largest group by atomic max (biased: group - BS_POD_GROUP_MISSING + 1, 0 = no row).  When an
//                    error word is set, nothing is written but kBaErrNode into the patch's error word: k_ba_merge then returns at once.
// Every kernel behind k_bb_rows returns at once when the wait core's or this header's error word is set: the block then has unwritten slots.
// S is a template parameter as for every kernel of this code object; request lanes move by unrolled constant-index loops, load to store:
// no register array, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_bound_apply.hpp"

namespace bs {

constexpr uint32_t kBbBlock = 1024;      // nodes per scan block
constexpr uint32_t kBbErrRange = 1u;     // a pod index >= the queue length (the host checks it first: never set in practice)
constexpr uint32_t kBbErrTwice = 2u;     // a pod index listed twice
constexpr uint32_t kBbErrNoNode = 4u;    // a pod the last pass gave no node
constexpr uint32_t kBbErrWaits = 8u;     // a pod that still waits in the pass's chains
constexpr uint32_t kBbErrNode = 16u;     // a row on a node >= n (the tables' own invariants: never set in practice)
enum : uint32_t { kBbResBa = 0, kBbResErr = 1, kBbResGroup = 2 };   // the result words: the patch's error word, this header's, the biased group maximum

struct BindDev {
  // the wait table's live rows (read only) and what the wait core's front half left
  const uint32_t* w_id;
  const int32_t* w_group;
  const uint32_t* w_node;
  const uint32_t* w_pres;
  const int64_t* w_req;       // [L][w_stride]
  uint32_t w_stride, W;       // W = 0 when no wait row is listed
  const uint32_t* mark;       // [mark_n] list position + 1 of a listed id
  uint32_t mark_n;
  const uint32_t* w_err;      // the wait core's error word (never null: a zero word when no wait row is listed)
  // the listed pods, the last pass's result block and its chains as an array
  const uint32_t* plist;      // [n_pod]
  const int32_t* pod_node;    // [P]
  const int32_t* wnode;       // [P] the node of a pod that still waits, else -1
  uint32_t* claim;            // [ceil(P / 32)] zeroed
  uint32_t n_wait, n_pod, n;  // n = n_wait + n_pod
  uint32_t P, N, ids;
  // the unsorted rows by slot
  uint32_t* u_node;
  int32_t* u_group;
  uint32_t* u_pres;
  int64_t* u_req;             // [L][n]
  // the host's blob by slot
  const int32_t* h_prio;
  const int64_t* h_start;
  const uint8_t* h_pdb;       // null = every bit clear
  // per node
  uint32_t* ncnt;             // [N] rows of the node, zeroed
  uint32_t* ncur;             // [N] the scatter's cursors, zeroed
  uint32_t* noff;             // [N + 1] segment starts
  uint32_t* bsum;             // [ceil(N / kBbBlock)]
  uint32_t* seg;              // [n] slots by node, arbitrary order within a node
  uint32_t* perm;             // [n] final position -> slot
  uint32_t* res;              // kBbRes* words, zeroed
  uint32_t* node_out;         // [n] by slot
  // the sorted block (BoundApplyDev's insert columns)
  uint32_t* inode;
  int32_t* iprio;
  int64_t* istart;
  int32_t* igroup;
  int64_t* ireq;              // [L][n]
  uint32_t* iid;
  uint32_t* ipres;
  uint8_t* ipdb;
};

__device__ __forceinline__ bool bb_failed(const BindDev& a) { return (*a.w_err | a.res[kBbResErr]) != 0u; }

template <int S>
__global__ __launch_bounds__(256) void k_bb_rows(BindDev a, PodsDev pd) {
  constexpr int L = 4 + S;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < a.W) {
    const uint32_t id = a.w_id[t];
    const uint32_t m = id < a.mark_n ? a.mark[id] : 0u;
    if (m != 0u && m - 1u < a.n_wait) {
      const uint32_t s = m - 1u, k = a.w_node[t];
      if (k >= a.N) {
        __hip_atomic_fetch_or(&a.res[kBbResErr], kBbErrNode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        a.u_node[s] = k;
        a.u_group[s] = a.w_group[t];
        a.u_pres[s] = a.w_pres[t];
#pragma unroll
        for (int l = 0; l < L; ++l) a.u_req[(size_t)l * a.n + s] = a.w_req[(size_t)l * a.w_stride + t];
        __hip_atomic_fetch_add(&a.ncnt[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (t < a.n_pod) {
    const uint32_t p = a.plist[t];
    uint32_t bad = 0;
    int32_t k = -1;
    if (p >= a.P || p >= pd.p) {
      bad = kBbErrRange;
    } else {
      const uint32_t bit = 1u << (p & 31u);
      if (__hip_atomic_fetch_or(&a.claim[p >> 5], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) bad = kBbErrTwice;
      k = a.pod_node[p];
      if (k < 0) bad |= kBbErrNoNode;
      else if (a.wnode[p] >= 0) bad |= kBbErrWaits;
      else if ((uint32_t)k >= a.N) bad |= kBbErrNode;
    }
    if (bad) {
      __hip_atomic_fetch_or(&a.res[kBbResErr], bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      const uint32_t s = a.n_wait + t;
      const uint32_t smask = S > 0 ? (uint32_t)((1ull << S) - 1ull) : 0u;
      const uint32_t pres = pd.pres[p] & smask;
      a.u_node[s] = (uint32_t)k;
      a.u_group[s] = pd.group[p];
      a.u_pres[s] = pres;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        int64_t v = 0;
        if (l < 3) v = pd.req[(size_t)l * pd.p + p];
        else if (l == 3) v = 1;
        else if ((pres >> (l - 4)) & 1u) v = pd.req[(size_t)l * pd.p + p];
        a.u_req[(size_t)l * a.n + s] = v;
      }
      __hip_atomic_fetch_add(&a.ncnt[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__device__ __forceinline__ uint32_t bb_wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

template <int S>
__global__ __launch_bounds__(kBbBlock) void k_bb_scan1(BindDev a) {
  __shared__ uint32_t s_w[kBbBlock / 64];
  const uint32_t t = threadIdx.x, k = blockIdx.x * kBbBlock + t;
  uint32_t v = k < a.N ? a.ncnt[k] : 0u;
  v = bb_wave_sum(v);
  if ((t & 63u) == 0u) s_w[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < kBbBlock / 64; ++w) s += s_w[w];
    a.bsum[blockIdx.x] = s;
  }
}

template <int S>
__global__ __launch_bounds__(kBbBlock) void k_bb_scan2(BindDev a) {
  __shared__ uint32_t s_w[kBbBlock / 64];
  __shared__ uint32_t s_x[kBbBlock / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6, k = blockIdx.x * kBbBlock + t;
  uint32_t pre = 0;                                         // the blocks in front of this one
  for (uint32_t b = t; b < blockIdx.x; b += kBbBlock) pre += a.bsum[b];
  pre = bb_wave_sum(pre);
  const uint32_t v = k < a.N ? a.ncnt[k] : 0u;
  uint32_t incl = v;                                        // inclusive inside the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)incl, off);
    if (lane >= (uint32_t)off) incl += u;
  }
  if (lane == 0) s_x[w] = pre;
  if (lane == 63u) s_w[w] = incl;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t j = 0; j < kBbBlock / 64; ++j) {
    base += s_x[j];
    if (j < w) base += s_w[j];
  }
  const uint32_t excl = base + incl - v;
  if (k < a.N) a.noff[k] = excl;
  if (k + 1u == a.N) a.noff[a.N] = excl + v;
}

template <int S>
__global__ __launch_bounds__(256) void k_bb_scatter(BindDev a) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= a.n || bb_failed(a)) return;
  const uint32_t k = a.u_node[s];
  if (k >= a.N) return;
  const uint32_t at = a.noff[k] + __hip_atomic_fetch_add(&a.ncur[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (at < a.n) a.seg[at] = s;
}

template <int S>
__global__ __launch_bounds__(256) void k_bb_rank(BindDev a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (k >= a.N || bb_failed(a)) return;
  const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ncnt[k]);
  if (cnt == 0u) return;
  const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.noff[k]);
  if (cnt > BS_BOUND_MAX_PER_NODE || s0 + cnt > a.n) {     // (survivors + inserts: k_ba_boff's check)
    if (lane == 0) __hip_atomic_fetch_or(&a.res[kBbResBa], kBaErrFull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  for (uint32_t base = 0; base < cnt; base += 64u) {
    const uint32_t i = base + lane;
    const bool have = i < cnt;
    const uint32_t s = have ? a.seg[s0 + i] : 0u;
    const int32_t p = have ? a.h_prio[s] : 0;
    const int64_t st = have ? a.h_start[s] : 0;
    uint32_t ahead = 0;
    for (uint32_t w = 0; w < cnt; w += 64u) {
      const uint32_t jw = w + lane;
      const uint32_t sj = jw < cnt ? a.seg[s0 + jw] : 0u;
      const int32_t pj = jw < cnt ? a.h_prio[sj] : 0;
      const int64_t stj = jw < cnt ? a.h_start[sj] : 0;
      const uint32_t m = min(64u, cnt - w);
      for (uint32_t x = 0; x < m; ++x) {
        const int32_t xp = __builtin_amdgcn_readlane(pj, (int)x);
        const int64_t xs = pre_readlane64(stj, x);
        const uint32_t xslot = (uint32_t)__builtin_amdgcn_readlane((int)sj, (int)x);
        ahead += (ba_before(xp, xs, p, st) || (xp == p && xs == st && xslot < s)) ? 1u : 0u;
      }
    }
    if (have) a.perm[s0 + ahead] = s;
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_bb_gather(BindDev a) {
  constexpr int L = 4 + S;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (bb_failed(a)) {
    if (r == 0u) __hip_atomic_fetch_or(&a.res[kBbResBa], kBaErrNode, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (a.res[kBbResBa] != 0u) return;                        // (k_bb_rank left a segment: perm[] has unwritten positions)
  uint32_t gb = 0;
  if (r < a.n) {
    const uint32_t s = a.perm[r];
    if (s < a.n) {
      const uint32_t k = a.u_node[s];
      const int32_t g = a.u_group[s];
      a.inode[r] = k;
      a.iprio[r] = a.h_prio[s];
      a.istart[r] = a.h_start[s];
      a.igroup[r] = g;
      a.iid[r] = a.ids + s;
      a.ipres[r] = a.u_pres[s];
      a.ipdb[r] = (a.h_pdb && a.h_pdb[s]) ? (uint8_t)1 : (uint8_t)0;
#pragma unroll
      for (int l = 0; l < L; ++l) a.ireq[(size_t)l * a.n + r] = a.u_req[(size_t)l * a.n + s];
      a.node_out[s] = k;
      gb = g >= BS_POD_GROUP_MISSING ? (uint32_t)(g - BS_POD_GROUP_MISSING) + 1u : 0u;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) gb = max(gb, (uint32_t)__shfl_xor((int)gb, off));
  if ((threadIdx.x & 63u) == 0u && gb) __hip_atomic_fetch_max(&a.res[kBbResGroup], gb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace bs
