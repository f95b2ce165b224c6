// bs_wait.hpp — the resident Permit-wait table: waiting pods that outlive their pass (bs_wait_park / _release / _expire / _forget).
//
// The pass (bs_seq.hpp) knows where its waiting pods sit for one cycle: the chain head[g] -> wait_rec[pod] in its scratch, keyed by queue
// index.  The reference's MatchedPodNodes (core.go:284-309) lives as long as the gang waits.  This table is that map, minus the clock:
// one row per waiting pod — id, group, node, the request lanes as the assume step counted them (pods lane 1, a scalar lane without a
// present bit 0), the present bits — in ascending id, in one allocation with a twin the compaction writes into.  tu_wait.hip alone emits
// the kernels (a unity build includes it); k_seq_pass and the k_se_* kernels are not touched.
//
// Kernels, handed over by launch boundary only (every value written in one launch is read in a later one):
//   k_wt_mark       one lane per listed group / id: mark[key] = list position + 1 by compare-and-swap from 0; a key that is marked already
//                   is listed twice -> the error word.  The mark arrays are zero between calls (k_wt_finish takes the marks off again).
//   k_wt_scan1      one lane per entry (a table row; in park mode a pod of the queue): "survives" and "leaves" packed in one 64-bit word
//                   (survives << 32 | leaves: both halves stay below 2^32, they never carry), summed per block of 1024.
//   k_wt_scan2      the spread scan's second half: the block totals in front of a block, an exclusive scan inside it; every entry's word is
//                   kept in pos[] (survivor position << 32 | output row).  The last entry writes the totals; in id mode fewer leaving rows
//                   than listed ids means a dead id -> the error word.
//   k_wt_move<S>    one thread per row, nothing on an error: a survivor is copied to its position in the twin; a leaving row writes
//                   (id, node) at its output row, counts itself for its listed group / reports its node for its listed id, and — expire and
//                   forget — adds its lanes into the per-node delta [L][N] (64-bit relaxed agent-scope atomic adds: wrapping sums commute),
//                   ORs its key bits into a per-node word, and appends the node to the dirty list if it touched it first.  forget: matched
//                   of its group falls by 1.  Lanes are indexed by unrolled constants only.
//   k_wt_nodes<S>   k_se_nodes' twin: one thread per dirty node writes the absolute bs_node_request record (base - delta; a scalar lane no
//                   leaving row has keeps its word and its bit; a lane one has loses the request and keeps its bit) for k_nodes_assume and
//                   returns the node's delta / bits / dirty words to zero.
//   k_wt_finish     one thread per list position: the mark comes off (also after an error); expire: unknown = matched - entries, matched = 0,
//                   BS_GROUP_DENIED when asked.
//   k_wt_walk       park: one lane per group follows its chain (k_se_walk's reading form): wnode[pod] = node.
//   k_wt_gather<S>  park: one thread per pod of the queue; a waiting pod writes its row at the table's tail (W + its rank in queue order):
//                   id = ids + rank, the request lanes from the resident queue, the node from the chain; and (pod, node) at row rank.
//   k_wt_chains     park: every chain becomes empty as k_se_groups leaves it (head 0, the count 0, kSeqHasRecord kept).
// The table follows node-list surgery (bs_wait_nodes_apply) by a fourth face of the same scan, kWtByNode; its two kernels carry another
// prefix because the k_wt_* set is counted (tests/test_wait_cpu.py):
//   k_wn_map        one lane per row: the one binary search of the call.  rem[] holds the removed OLD nodes, ascending; lo = how many lie
//                   below the row's node k.  nnode[e] = kWtGone when k itself is listed, else k - lo, the node's new index.  k_wt_scan1 /
//                   k_wt_scan2 and the move read nnode[], they do not search again.
//   k_wn_move<S>    one thread per row: a survivor is copied to its position in the twin with nnode[e] in the node column; a leaving row
//                   writes (id, OLD node, group) at its output row and takes 1 off matched of its group (a relaxed agent-scope atomic:
//                   many rows of one group leave from many blocks).  No marks, no node side: the node is gone.
#pragma once

#include "bs_seq.hpp"

namespace bs {

constexpr uint32_t kWtBlock = 1024;   // entries per scan block
enum : uint32_t { kWtByGroup = 0, kWtById = 1, kWtPark = 2, kWtByNode = 3 };
constexpr uint32_t kWtGone = 0xFFFFFFFFu;   // nnode[e] of a row whose node was removed (a node index stays below the node count)
enum : uint32_t { kWtKept = 0, kWtLeft = 1, kWtDirty = 2, kWtErr = 3 };   // info words
enum : uint32_t { kWtErrTwice = 1, kWtErrDead = 2 };

// the table's columns in one allocation; req is [L][stride]
struct WaitTab {
  uint32_t* id;
  int32_t* group;
  uint32_t* node;
  uint32_t* pres;
  int64_t* req;
  uint32_t stride;
};

struct WaitDev {
  WaitTab src, dst;                     // the live table, and the twin the compaction writes (park: src only, its tail is written)
  uint32_t W;                           // rows of src
  uint32_t E;                           // entries the scan runs over: W, or the queue length in park mode
  uint32_t mode;                        // kWtByGroup / kWtById / kWtPark / kWtByNode
  // the call
  const uint32_t* list;                 // [M] listed groups or ids
  uint32_t M;
  uint32_t* mark;                       // [mark_n] list position + 1 of a listed key, zero between calls
  uint32_t mark_n;                      // G, or the id space
  uint32_t node_side, forget, expire, deny;
  // scratch
  unsigned long long* bsum;             // [cdiv(E, kWtBlock)] block totals
  unsigned long long* pos;              // [E] exclusive scan: survivor position << 32 | output row
  uint32_t* info;                       // kWtKept, kWtLeft, kWtDirty, kWtErr (zeroed before the launches)
  uint32_t* o_key; uint32_t* o_node;    // [E] the rows: (id, node), park: (pod, node)
  uint32_t* l_cnt;                      // [M] rows that left per listed group (zeroed before the launches)
  uint32_t* l_out;                      // [M] expire: matched - entries per listed group; forget: the node of each listed id
  // the node side
  unsigned long long* delta;            // [L][N], zero between calls
  uint32_t* nbits;                      // [N] scalar keys the leaving rows of a node have, zero between calls
  uint32_t* dirty;                      // [N] zero between calls
  uint32_t* dlist;                      // [min(N, W)]
  uint32_t N;
  // the groups
  uint32_t* g_matched;                  // [G]
  uint8_t* g_flags;                     // [G]
  uint32_t G;
  // park: the pass's waiting state (bs_seq.hpp, SeqDev)
  const unsigned long long* wait_rec;   // [P]
  uint32_t* head;                       // [G]
  uint32_t* nwait;                      // [G]
  int32_t* wnode;                       // [P] filled with -1, then the chains' nodes
  uint32_t P, ids;
  // by node: the removed OLD nodes, and what k_wn_map decided per row
  const uint32_t* rem;                  // [R] ascending, distinct
  uint32_t R;
  uint32_t* nnode;                      // [W] the row's new node index, kWtGone when its node is removed
  int32_t* o_group;                     // [W] the third column of the rows (the removal core: NULL unless the caller wants it)
};

// survives << 32 | leaves
__device__ __forceinline__ unsigned long long wt_entry(const WaitDev& a, uint32_t e) {
  bool leaves;
  if (a.mode == kWtPark) {
    leaves = a.wnode[e] >= 0;
  } else if (a.mode == kWtByNode) {
    leaves = a.nnode[e] == kWtGone;
  } else {
    const uint32_t key = a.mode == kWtById ? a.src.id[e] : (uint32_t)a.src.group[e];
    leaves = key < a.mark_n && a.mark[key] != 0u;
  }
  return leaves ? 1ull : (1ull << 32);
}

__device__ __forceinline__ unsigned long long wt_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
  return v;
}

__global__ __launch_bounds__(256) void k_wt_mark(WaitDev a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.M) return;
  const uint32_t key = a.list[i];
  if (key >= a.mark_n) return;                              // (the host has refused such a list)
  if (atomicCAS(&a.mark[key], 0u, i + 1u) != 0u) __hip_atomic_fetch_or(&a.info[kWtErr], kWtErrTwice, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kWtBlock) void k_wt_scan1(WaitDev a) {
  __shared__ unsigned long long s_w[kWtBlock / 64];
  const uint32_t t = threadIdx.x, e = blockIdx.x * kWtBlock + t;
  unsigned long long v = e < a.E ? wt_entry(a, e) : 0ull;
  v = wt_wave_sum(v);
  if ((t & 63u) == 0u) s_w[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    unsigned long long s = 0;
    for (uint32_t w = 0; w < kWtBlock / 64; ++w) s += s_w[w];
    a.bsum[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kWtBlock) void k_wt_scan2(WaitDev a) {
  __shared__ unsigned long long s_w[kWtBlock / 64];
  __shared__ unsigned long long s_x[kWtBlock / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6, e = blockIdx.x * kWtBlock + t;
  unsigned long long pre = 0;                               // the blocks in front of this one
  for (uint32_t b = t; b < blockIdx.x; b += kWtBlock) pre += a.bsum[b];
  pre = wt_wave_sum(pre);
  const unsigned long long v = e < a.E ? wt_entry(a, e) : 0ull;
  unsigned long long incl = v;                              // inclusive inside the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long u = (unsigned long long)__shfl_up((long long)incl, off);
    if (lane >= (uint32_t)off) incl += u;
  }
  if (lane == 0) s_x[w] = pre;
  if (lane == 63u) s_w[w] = incl;
  __syncthreads();
  unsigned long long base = 0;
  for (uint32_t k = 0; k < kWtBlock / 64; ++k) {
    base += s_x[k];
    if (k < w) base += s_w[k];
  }
  const unsigned long long excl = base + incl - v;
  if (e < a.E) a.pos[e] = excl;
  if (e + 1u == a.E) {
    const unsigned long long tot = excl + v;
    a.info[kWtKept] = (uint32_t)(tot >> 32);
    a.info[kWtLeft] = (uint32_t)tot;
    if (a.mode == kWtById && (uint32_t)tot != a.M)          // distinct ids mark at most one row each: fewer rows than ids = a dead id
      __hip_atomic_fetch_or(&a.info[kWtErr], kWtErrDead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_wt_move(WaitDev a) {
  constexpr int L = 4 + S;
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= a.W || a.info[kWtErr]) return;
  const unsigned long long at = a.pos[e];
  const uint32_t id = a.src.id[e], k = a.src.node[e], pres = a.src.pres[e];
  const int32_t g = a.src.group[e];
  const uint32_t key = a.mode == kWtById ? id : (uint32_t)g;
  const uint32_t m = key < a.mark_n ? a.mark[key] : 0u;
  if (!m) {                                                 // a survivor: the same columns, its position in the twin
    const uint32_t d = (uint32_t)(at >> 32);
    if (d >= a.dst.stride) return;
    a.dst.id[d] = id;
    a.dst.group[d] = g;
    a.dst.node[d] = k;
    a.dst.pres[d] = pres;
#pragma unroll
    for (int l = 0; l < L; ++l) a.dst.req[(size_t)l * a.dst.stride + d] = a.src.req[(size_t)l * a.src.stride + e];
    return;
  }
  const uint32_t row = (uint32_t)at;
  if (row < a.W) {
    a.o_key[row] = id;
    a.o_node[row] = k;
    if (a.o_group) a.o_group[row] = g;                      // (bs_groups_list_apply's release: the group leaves with its rows)
  }
  if (m - 1u < a.M) {
    if (a.mode == kWtById) a.l_out[m - 1u] = k;
    else __hip_atomic_fetch_add(&a.l_cnt[m - 1u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!a.node_side || k >= a.N) return;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const unsigned long long v = (unsigned long long)a.src.req[(size_t)l * a.src.stride + e];
    if (v) __hip_atomic_fetch_add(&a.delta[(size_t)l * a.N + k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (pres) __hip_atomic_fetch_or(&a.nbits[k], pres, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__hip_atomic_exchange(&a.dirty[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
    const uint32_t slot = __hip_atomic_fetch_add(&a.info[kWtDirty], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.dlist[slot] = k;                                      // (a node enters once: at most min(N, W) entries)
  }
  if (a.forget && (uint32_t)g < a.G) __hip_atomic_fetch_add(&a.g_matched[g], 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int S>
__global__ __launch_bounds__(256) void k_wt_nodes(WaitDev a, const int64_t* nreq, const uint32_t* rpres, uint32_t nstride, bs_node_request* out) {
  constexpr int L = 4 + S;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.info[kWtDirty]) return;
  const uint32_t k = a.dlist[i];
  const uint32_t rp = rpres[k], touched = a.nbits[k];
  bs_node_request r;
  r.index = k;
  r.requested_present = rp | touched;
#pragma unroll
  for (int l = 0; l < BS_MAX_LANES; ++l) r.requested[l] = 0;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int64_t raw = nreq[(size_t)l * nstride + k];
    const bool lane_on = l < 4 || ((touched >> (l - 4)) & 1u);
    if (!lane_on) { r.requested[l] = raw; continue; }
    const int64_t base = (l < 4 || ((rp >> (l - 4)) & 1u)) ? raw : 0;
    r.requested[l] = wsub(base, (int64_t)a.delta[(size_t)l * a.N + k]);
    a.delta[(size_t)l * a.N + k] = 0ull;
  }
  a.nbits[k] = 0u;
  a.dirty[k] = 0u;
  out[i] = r;
}

__global__ __launch_bounds__(256) void k_wt_finish(WaitDev a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.M) return;
  const uint32_t key = a.list[i];
  if (key >= a.mark_n) return;
  a.mark[key] = 0u;
  if (!a.expire || a.info[kWtErr] || key >= a.G) return;
  a.l_out[i] = a.g_matched[key] - a.l_cnt[i];
  a.g_matched[key] = 0u;
  if (a.deny) a.g_flags[key] = (uint8_t)(a.g_flags[key] | BS_GROUP_DENIED);
}

__global__ __launch_bounds__(256) void k_wt_walk(WaitDev a) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= a.G) return;
  const uint32_t cnt = a.nwait[s] & ~kSeqHasRecord;
  uint32_t h = a.head[s];
  for (uint32_t step = 0; step < cnt && h != 0u && h - 1u < a.P; ++step) {
    const unsigned long long rec = a.wait_rec[h - 1u];
    a.wnode[h - 1u] = (int32_t)(uint32_t)rec;
    h = (uint32_t)(rec >> 32);
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_wt_gather(WaitDev a, PodsDev pd) {
  constexpr int L = 4 + S;
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= a.P || p >= pd.p) return;
  const int32_t k = a.wnode[p];
  if (k < 0) return;
  const uint32_t rank = (uint32_t)a.pos[p], d = a.W + rank;
  if (d >= a.src.stride || rank >= a.P) return;
  const uint32_t smask = S > 0 ? (uint32_t)((1ull << S) - 1ull) : 0u;
  const uint32_t pres = pd.pres[p] & smask;
  a.src.id[d] = a.ids + rank;
  a.src.group[d] = pd.group[p];
  a.src.node[d] = (uint32_t)k;
  a.src.pres[d] = pres;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    int64_t v = 0;
    if (l < 3) v = pd.req[(size_t)l * pd.p + p];
    else if (l == 3) v = 1;
    else if ((pres >> (l - 4)) & 1u) v = pd.req[(size_t)l * pd.p + p];
    a.src.req[(size_t)l * a.src.stride + d] = v;
  }
  a.o_key[rank] = p;
  a.o_node[rank] = (uint32_t)k;
}

__global__ __launch_bounds__(256) void k_wt_chains(WaitDev a) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= a.G) return;
  a.head[s] = 0u;
  a.nwait[s] = a.nwait[s] & kSeqHasRecord;
}

__global__ __launch_bounds__(256) void k_wn_map(WaitDev a) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= a.W) return;
  const uint32_t k = a.src.node[e];
  uint32_t lo = 0, hi = a.R;                                // the first j with rem[j] >= k: the removed nodes below k
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.rem[mid] < k) lo = mid + 1u;
    else hi = mid;
  }
  a.nnode[e] = (lo < a.R && a.rem[lo] == k) ? kWtGone : k - lo;
}

template <int S>
__global__ __launch_bounds__(256) void k_wn_move(WaitDev a) {
  constexpr int L = 4 + S;
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= a.W) return;
  const unsigned long long at = a.pos[e];
  const uint32_t id = a.src.id[e], nn = a.nnode[e];
  const int32_t g = a.src.group[e];
  if (nn != kWtGone) {                                      // a survivor: the same columns but the node, its position in the twin
    const uint32_t d = (uint32_t)(at >> 32);
    if (d >= a.dst.stride) return;
    a.dst.id[d] = id;
    a.dst.group[d] = g;
    a.dst.node[d] = nn;
    a.dst.pres[d] = a.src.pres[e];
#pragma unroll
    for (int l = 0; l < L; ++l) a.dst.req[(size_t)l * a.dst.stride + d] = a.src.req[(size_t)l * a.src.stride + e];
    return;
  }
  const uint32_t row = (uint32_t)at;
  if (row < a.W) { a.o_key[row] = id; a.o_node[row] = a.src.node[e]; a.o_group[row] = g; }
  if ((uint32_t)g < a.G) __hip_atomic_fetch_add(&a.g_matched[g], 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace bs
