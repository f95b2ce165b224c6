// bs_seq_expire.hpp — a gang's Permit timeout, undone on the device (bs_seq_expire, bs_seq_waiting_read).
//
// What the reference does when a gang's PodNameUIDs entry runs out (controller.go:322-332): OnEvicted rejects every entry of
// MatchedPodNodes (batchscheduler.go:346-352), the framework unreserves each pod and the cache forgets it (NodeInfo.RemovePod), the
// entries are deleted (:328) and the group goes onto the deny list (:332 -> core.go:422-425).  The pass (bs_seq.hpp) leaves the only
// record of where its waiting pods sit in its own scratch: per gang the chain head[g] -> wait_rec[pod] = (next + 1) << 32 | node, last
// waiting pod first, and the count nwait[g] & ~kSeqHasRecord.  That scratch is READ here; k_seq_pass is not touched.  tu_seq_expire.hip
// alone emits the kernels (a unity build includes it).
//
// Kernels, handed over by launch boundary only (every value written in one launch is read in a later one):
//   k_se_scan1      one lane per entry (a listed group, or every group in ALL mode): the entry's pod count and "is kept" bit packed in one
//                   64-bit word (kept << 32 | pods: the pods of all entries together are at most P < 2^32, so the halves never carry),
//                   summed per block of 1024.
//   k_se_scan2      the spread scan's second half: the block totals in front of a block, an exclusive scan inside it; a kept entry writes
//                   its group, its pod count, matched - pods (uint32) and its row offset at its slot (ALL mode compacts: ascending index).
//   k_se_walk       one lane per kept slot follows the gang's chain and writes (pod, node) at offset + count - 1 - step: rows ascend by
//                   queue index.  The hops are dependent loads: a timeout is an event on a scale of seconds and gangs walk in parallel.
//                   With a wait_node array it serves bs_seq_waiting_read instead: one lane per group, wait_node[pod] = node, nothing else.
//   k_se_sum<S>     one thread per forgotten pod: its request lanes into the per-node delta [L][N] (64-bit relaxed agent-scope atomic adds:
//                   wrapping sums commute), its scalar-key bits ORed into a per-node word; the thread that touches a node first appends
//                   it to the dirty list.  Lanes are indexed by unrolled constants only (registers, no scratch).
//   k_se_nodes<S>   one thread per dirty node: its absolute request record by k_pc_nodes' rule (base - delta; a scalar lane no forgotten
//                   pod has keeps its word and its bit; a lane one has loses the request and keeps its bit) for k_nodes_assume, and the
//                   node's delta / bits / dirty words return to zero (the scratch is born zeroed and stays so between calls).
//   k_se_groups     one thread per expired group: matched = 0, BS_GROUP_DENIED when asked, the chain becomes empty (kSeqHasRecord stays).
#pragma once

#include "bs_seq.hpp"

namespace bs {

constexpr uint32_t kSeBlock = 1024;   // entries per scan block

struct SeqExpireDev {
  // the pass's waiting state (bs_seq.hpp, SeqDev) and what it indexes
  const unsigned long long* wait_rec;   // [P]
  uint32_t* head;                       // [G]
  uint32_t* nwait;                      // [G]
  uint32_t P, G;
  uint32_t* g_matched;                  // [G]
  uint8_t* g_flags;                     // [G]
  // the call
  const uint32_t* list;                 // [M] the listed groups; nullptr = ALL mode, entry e is group e
  uint32_t M;                           // entries: the list's length, or G
  uint32_t deny;
  // scratch
  unsigned long long* bsum;             // [cdiv(M, kSeBlock)] block totals, kept << 32 | pods
  uint32_t* info;                       // [0] groups expired [1] pods forgotten [2] dirty nodes (zeroed before the launches)
  uint32_t* o_group; uint32_t* o_gpods; uint32_t* o_gearlier; uint32_t* o_off;   // [M] per kept slot
  uint32_t* o_pod; uint32_t* o_node;    // [P] the rows
  // the node side
  unsigned long long* delta;            // [L][N], zero between calls
  uint32_t* nbits;                      // [N] scalar keys the forgotten pods of a node have, zero between calls
  uint32_t* dirty;                      // [N] zero between calls
  uint32_t* dlist;                      // [min(N, P)]
  uint32_t N;
};

__device__ __forceinline__ unsigned long long se_entry(const SeqExpireDev& a, uint32_t e, uint32_t& g) {
  g = a.list ? a.list[e] : e;
  const uint32_t cnt = a.nwait[g] & ~kSeqHasRecord;
  const uint32_t keep = (a.list || cnt) ? 1u : 0u;
  return ((unsigned long long)keep << 32) | cnt;
}

__device__ __forceinline__ unsigned long long se_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
  return v;
}

__global__ __launch_bounds__(kSeBlock) void k_se_scan1(SeqExpireDev a) {
  __shared__ unsigned long long s_w[kSeBlock / 64];
  const uint32_t t = threadIdx.x, e = blockIdx.x * kSeBlock + t;
  uint32_t g;
  unsigned long long v = e < a.M ? se_entry(a, e, g) : 0ull;
  v = se_wave_sum(v);
  if ((t & 63u) == 0u) s_w[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    unsigned long long s = 0;
    for (uint32_t w = 0; w < kSeBlock / 64; ++w) s += s_w[w];
    a.bsum[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kSeBlock) void k_se_scan2(SeqExpireDev a) {
  __shared__ unsigned long long s_w[kSeBlock / 64];
  __shared__ unsigned long long s_x[kSeBlock / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6, e = blockIdx.x * kSeBlock + t;
  unsigned long long pre = 0;                               // the blocks in front of this one
  for (uint32_t b = t; b < blockIdx.x; b += kSeBlock) pre += a.bsum[b];
  pre = se_wave_sum(pre);
  uint32_t g = 0;
  const unsigned long long v = e < a.M ? se_entry(a, e, g) : 0ull;
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
  for (uint32_t k = 0; k < kSeBlock / 64; ++k) {
    base += s_x[k];
    if (k < w) base += s_w[k];
  }
  const unsigned long long excl = base + incl - v;
  if (e < a.M && (v >> 32)) {
    const uint32_t slot = (uint32_t)(excl >> 32), cnt = (uint32_t)v;
    a.o_group[slot] = g;
    a.o_gpods[slot] = cnt;
    a.o_gearlier[slot] = a.g_matched[g] - cnt;
    a.o_off[slot] = (uint32_t)excl;
  }
  if (e + 1u == a.M) {
    const unsigned long long tot = excl + v;
    a.info[0] = (uint32_t)(tot >> 32);
    a.info[1] = (uint32_t)tot;
  }
}

__global__ __launch_bounds__(256) void k_se_walk(SeqExpireDev a, int32_t* wait_node) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (wait_node) {                                          // bs_seq_waiting_read: every group's chain, nothing else is written
    if (s >= a.G) return;
    const uint32_t cnt = a.nwait[s] & ~kSeqHasRecord;
    uint32_t h = a.head[s];
    for (uint32_t step = 0; step < cnt && h != 0u && h - 1u < a.P; ++step) {
      const unsigned long long rec = a.wait_rec[h - 1u];
      wait_node[h - 1u] = (int32_t)(uint32_t)rec;
      h = (uint32_t)(rec >> 32);
    }
    return;
  }
  if (s >= a.M || s >= a.info[0]) return;
  const uint32_t g = a.o_group[s], cnt = a.o_gpods[s], off = a.o_off[s];
  uint32_t h = a.head[g];
  for (uint32_t step = 0; step < cnt && h != 0u && h - 1u < a.P; ++step) {
    const unsigned long long rec = a.wait_rec[h - 1u];
    const uint32_t row = off + cnt - 1u - step;
    if (row < a.P) { a.o_pod[row] = h - 1u; a.o_node[row] = (uint32_t)rec; }
    h = (uint32_t)(rec >> 32);
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_se_sum(SeqExpireDev a, PodsDev pd) {
  constexpr int L = 4 + S;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= a.P || r >= a.info[1]) return;
  const uint32_t p = a.o_pod[r], k = a.o_node[r];
  if (p >= pd.p || k >= a.N) return;
  const uint32_t smask = S > 0 ? (uint32_t)((1ull << S) - 1ull) : 0u;
  const uint32_t pres = pd.pres[p] & smask;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    unsigned long long v = 0;
    if (l < 3) v = (unsigned long long)pd.req[(size_t)l * pd.p + p];
    else if (l == 3) v = 1ull;
    else if ((pres >> (l - 4)) & 1u) v = (unsigned long long)pd.req[(size_t)l * pd.p + p];
    if (v) __hip_atomic_fetch_add(&a.delta[(size_t)l * a.N + k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (pres) __hip_atomic_fetch_or(&a.nbits[k], pres, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__hip_atomic_exchange(&a.dirty[k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
    const uint32_t at = __hip_atomic_fetch_add(&a.info[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.dlist[at] = k;                                        // (a node enters once: at most min(N, P) entries)
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_se_nodes(SeqExpireDev a, const int64_t* nreq, const uint32_t* rpres, uint32_t nstride, bs_node_request* out) {
  constexpr int L = 4 + S;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.info[2]) return;
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

__global__ __launch_bounds__(256) void k_se_groups(SeqExpireDev a) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= a.M || s >= a.info[0]) return;
  const uint32_t g = a.o_group[s];
  a.g_matched[g] = 0u;
  if (a.deny) a.g_flags[g] = (uint8_t)(a.g_flags[g] | BS_GROUP_DENIED);
  a.head[g] = 0u;
  a.nwait[g] = a.nwait[g] & kSeqHasRecord;
}

}  // namespace bs
