// bs_bound_apply.hpp — the resident bound-pod table patched in place (include/bsched.h, bs_bound_apply): entries leave by id, new
// entries arrive with fresh ids, and every node's list stays in the load's importance order (priority descending, start ascending, id
// ascending).  Host work is O(delta): the inserts sorted by (node, importance) and packed with the remove ids into one blob.  The device
// makes one pass over the table into the second allocation (CompactDev, as BS_PREEMPT_APPLY), which the host swaps in once the error word
// came back clear.
//
// Four launches (plain loads and stores, atomics on the scratch words; hand-over between kernels by launch boundaries only):
//   k_ba_scatter<S>  pos_of[id[j]] = j over the live table (pos_of: id space, pre-filled with 0xffffffff).
//   k_ba_mark<S>     one thread per remove id: unknown / not live / listed twice go into the error word, otherwise the position's bit in
//                    the dead mask is claimed (atomic or: a second claim is the duplicate) and the node's dead count rises (its node by a
//                    binary search of the CSR offsets).  One thread per insert: the node's insert count, and the segment's first index.
//   k_ba_boff<S>     one block: len'[k] = len[k] - dead[k] + inserts[k], the per-node capacity check into the error word, exclusive scan:
//                    the new CSR (k_pc_boff's scan).
//   k_ba_merge<S>    one wave per node, four nodes per workgroup; returns at once when the error word is set (the lengths it would write by
//                    are then not the ones the target was sized for).  An untouched node is a straight coalesced copy.  Otherwise the
//                    survivors are compacted stably by ballot (k_pc_compact's loop) and merged with the node's sorted insert segment by
//                    rank counting, 64 entries per step: a survivor moves back by the inserts strictly more important in (priority,
//                    start), an insert lands at its rank in the segment plus the survivors at least as important (an insert's id is
//                    larger than every survivor's, so a tie goes behind).  Every column moves; lane 0 writes the node's PDB count.
// With BS_BOUND_NODES (bs_bound_apply_ex) a fifth launch follows once the host has read the error word clear:
//   k_ba_nodes<S>    one wave per node, four nodes per workgroup; a node the delta does not touch returns at once.  The lanes stride over
//                    the node's OLD list (still intact: the merge wrote the other allocation) and subtract the entries whose dead bit is
//                    set, then over the node's insert segment and add; a wave reduction, and lane 0 writes the node's new absolute
//                    request vector (k_pc_nodes' rule) as a bs_node_request record at a slot taken from a counter.  k_nodes_assume runs
//                    over the records.
// S is a template parameter as for every kernel of this code object (one symbol per translation unit that instantiates it); the request
// lanes are moved by an unrolled loop, load to store: no register array, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_preempt_commit.hpp"

namespace bs {

constexpr uint32_t kBaErrUnknown = 1u;   // a remove id >= the id space
constexpr uint32_t kBaErrDead = 2u;      // a remove id that is not live
constexpr uint32_t kBaErrTwice = 4u;     // a remove id listed twice
constexpr uint32_t kBaErrNode = 8u;      // an insert on a node >= n (the host checks it first: never set in practice)
constexpr uint32_t kBaErrFull = 16u;     // a node over BS_BOUND_MAX_PER_NODE after the delta
constexpr uint32_t kBaNone = 0xffffffffu;

struct BoundApplyDev {
  // the live table (read only here)
  const uint32_t* boff;
  const int32_t* bprio;
  const int64_t* bstart;
  const int32_t* bgroup;
  const int64_t* breq;      // [L][bstride]
  const uint32_t* bid;
  const uint32_t* bpres;
  const uint8_t* bpdb;
  uint32_t bstride, b, n, ids;
  // the delta: remove ids, and the inserts sorted by (node, importance), columns as the table's
  uint32_t n_remove, n_insert;
  const uint32_t* rem;
  const uint32_t* inode;
  const int32_t* iprio;
  const int64_t* istart;
  const int32_t* igroup;
  const int64_t* ireq;      // [L][n_insert]
  const uint32_t* iid;
  const uint32_t* ipres;
  const uint8_t* ipdb;
  // scratch of this call
  uint32_t* pos_of;         // [ids] table position of each live id (0xffffffff before the scatter)
  uint32_t* deadw;          // [ceil(b / 32)] one bit per table position, zeroed
  uint32_t* dcnt;           // [n] removed entries of the node, zeroed
  uint32_t* icnt;           // [n] inserted entries of the node, zeroed
  uint32_t* ifirst;         // [n] first index of the node's insert segment (where icnt != 0)
  uint32_t* err;            // kBaErr* bits, zeroed
};

template <int S>
__global__ __launch_bounds__(256) void k_ba_scatter(BoundApplyDev a) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= a.b) return;
  const uint32_t id = a.bid[j];
  if (id < a.ids) a.pos_of[id] = j;
}

template <int S>
__global__ __launch_bounds__(256) void k_ba_mark(BoundApplyDev a) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < a.n_remove) {
    const uint32_t id = a.rem[t];
    const uint32_t pos = id < a.ids ? a.pos_of[id] : kBaNone;
    if (pos >= a.b) {
      atomicOr(a.err, id < a.ids ? kBaErrDead : kBaErrUnknown);
    } else {
      const uint32_t bit = 1u << (pos & 31u);
      if (atomicOr(a.deadw + (pos >> 5), bit) & bit) {
        atomicOr(a.err, kBaErrTwice);
      } else {
        uint32_t lo = 0, hi = a.n;                       // the first k with boff[k] > pos (boff[n] = b > pos): the node is k - 1
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (a.boff[mid] <= pos) lo = mid + 1u;
          else hi = mid;
        }
        atomicAdd(a.dcnt + (lo - 1u), 1u);
      }
    }
  }
  if (t < a.n_insert) {
    const uint32_t k = a.inode[t];
    if (k >= a.n) {
      atomicOr(a.err, kBaErrNode);
    } else {
      atomicAdd(a.icnt + k, 1u);
      if (t == 0 || a.inode[t - 1] != k) a.ifirst[k] = t;
    }
  }
}

// the new CSR offsets, one block (k_pc_boff's scan over len - dead + inserts)
template <int S>
__global__ __launch_bounds__(1024) void k_ba_boff(BoundApplyDev a, uint32_t* nboff) {
  __shared__ uint32_t s_part[1024];
  const uint32_t t = threadIdx.x, n = a.n;
  const uint32_t per = (n + 1023u) / 1024u, k0 = min(n, t * per), k1 = min(n, k0 + per);
  uint32_t sum = 0;
  bool full = false;
  for (uint32_t k = k0; k < k1; ++k) {
    const uint32_t len = (a.boff[k + 1] - a.boff[k]) - a.dcnt[k] + a.icnt[k];
    full |= len > BS_BOUND_MAX_PER_NODE;
    sum += len;
  }
  if (full) atomicOr(a.err, kBaErrFull);
  s_part[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {       // inclusive scan (Hillis-Steele)
    const uint32_t v = t >= off ? s_part[t - off] : 0u;
    __syncthreads();
    s_part[t] += v;
    __syncthreads();
  }
  uint32_t run = t ? s_part[t - 1] : 0u;
  for (uint32_t k = k0; k < k1; ++k) {
    nboff[k] = run;
    run += (a.boff[k + 1] - a.boff[k]) - a.dcnt[k] + a.icnt[k];
  }
  if (t == 1023u) nboff[n] = s_part[1023];
}

// a is strictly more important than b in (priority, start)
__device__ __forceinline__ bool ba_before(int32_t pa, int64_t sa, int32_t pb, int64_t sb) { return pa > pb || (pa == pb && sa < sb); }

template <int S>
__device__ __forceinline__ void ba_move_old(const BoundApplyDev& a, const CompactDev& nw, uint32_t j, uint32_t d, uint8_t pdb) {
  constexpr int L = 4 + S;
  nw.bprio[d] = a.bprio[j];
  nw.bstart[d] = a.bstart[j];
  nw.bgroup[d] = a.bgroup[j];
  nw.bid[d] = a.bid[j];
  nw.bpres[d] = a.bpres[j];
  nw.bpdb[d] = pdb;
#pragma unroll
  for (int l = 0; l < L; ++l) nw.breq[(size_t)l * nw.bstride + d] = a.breq[(size_t)l * a.bstride + j];
}

template <int S>
__global__ __launch_bounds__(256) void k_ba_merge(BoundApplyDev a, CompactDev nw) {
  constexpr int L = 4 + S;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (k >= a.n || *a.err != 0u) return;
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[k]), b1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[k + 1]);
  const uint32_t nd = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.dcnt[k]), ni = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.icnt[k]);
  const uint32_t dst0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)nw.boff[k]);
  uint32_t nviol = 0;
  if (nd == 0u && ni == 0u) {                              // untouched: the list moves as it is
    for (uint32_t base = b0; base < b1; base += 64u) {
      const uint32_t j = base + lane;
      const bool in = j < b1;
      const uint8_t pdb = in ? a.bpdb[j] : (uint8_t)0;
      nviol += (uint32_t)__builtin_popcountll(__ballot(pdb != 0));
      if (in) ba_move_old<S>(a, nw, j, dst0 + (j - b0), pdb);
    }
    if (lane == 0) nw.bnviol[k] = nviol;
    return;
  }
  const uint32_t i0 = ni ? (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ifirst[k]) : 0u;
  // the survivors, in table order: each behind the inserts that are strictly more important
  uint32_t sbase = 0;
  for (uint32_t base = b0; base < b1; base += 64u) {
    const uint32_t j = base + lane;
    const bool keep = j < b1 && !((a.deadw[j >> 5] >> (j & 31u)) & 1u);
    const uint64_t m = __ballot(keep);
    if (!m) continue;
    const int32_t p = keep ? a.bprio[j] : 0;
    const int64_t st = keep ? a.bstart[j] : 0;
    const uint8_t pdb = keep ? a.bpdb[j] : (uint8_t)0;
    uint32_t ahead = 0;
    for (uint32_t w = 0; w < ni; w += 64u) {
      const uint32_t iw = w + lane;
      const int32_t ip = iw < ni ? a.iprio[i0 + iw] : 0;
      const int64_t is = iw < ni ? a.istart[i0 + iw] : 0;
      const uint32_t cnt = min(64u, ni - w);
      for (uint32_t x = 0; x < cnt; ++x)
        ahead += ba_before(__builtin_amdgcn_readlane(ip, (int)x), pre_readlane64(is, x), p, st) ? 1u : 0u;
    }
    nviol += (uint32_t)__builtin_popcountll(__ballot(pdb != 0));
    const uint32_t rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (keep) ba_move_old<S>(a, nw, j, dst0 + sbase + rank + ahead, pdb);
    sbase += (uint32_t)__builtin_popcountll(m);
  }
  // the inserts, in segment order: each behind the survivors that are at least as important
  for (uint32_t w = 0; w < ni; w += 64u) {
    const uint32_t iw = w + lane, src = i0 + iw;
    const bool have = iw < ni;
    const int32_t ip = have ? a.iprio[src] : 0;
    const int64_t is = have ? a.istart[src] : 0;
    uint32_t ahead = 0;
    for (uint32_t base = b0; base < b1; base += 64u) {
      const uint32_t j = base + lane;
      const bool keep = j < b1 && !((a.deadw[j >> 5] >> (j & 31u)) & 1u);
      uint64_t m = __ballot(keep);
      if (!m) continue;
      const int32_t p = keep ? a.bprio[j] : 0;
      const int64_t st = keep ? a.bstart[j] : 0;
      while (m) {
        const uint32_t x = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        ahead += ba_before(ip, is, __builtin_amdgcn_readlane(p, (int)x), pre_readlane64(st, x)) ? 0u : 1u;
      }
    }
    const uint8_t pdb = have ? a.ipdb[src] : (uint8_t)0;
    nviol += (uint32_t)__builtin_popcountll(__ballot(pdb != 0));
    if (have) {
      const uint32_t d = dst0 + iw + ahead;
      nw.bprio[d] = ip;
      nw.bstart[d] = is;
      nw.bgroup[d] = a.igroup[src];
      nw.bid[d] = a.iid[src];
      nw.bpres[d] = a.ipres[src];
      nw.bpdb[d] = pdb;
#pragma unroll
      for (int l = 0; l < L; ++l) nw.breq[(size_t)l * nw.bstride + d] = a.ireq[(size_t)l * a.n_insert + src];
    }
  }
  if (lane == 0) nw.bnviol[k] = nviol;
}

// what k_ba_nodes reads of the node table and where its records go
struct BoundNodesReqDev {
  const int64_t* nreq;      // [L][nstride] the nodes' requested lanes
  const uint32_t* rpres;    // [n] their present bits
  uint32_t nstride;
  uint32_t cap;             // records `out` holds: min(n, n_remove + n_insert), which bounds the touched nodes
  uint32_t* count;          // zeroed; the number of records written
  bs_node_request* out;
};

// BS_BOUND_NODES: node k gets requested - (its removed entries) + (its inserted entries), wrapping; a scalar lane none of them has keeps
// its word and its present bit, the others are set (an absent key counts as 0): k_pc_nodes' rule.  The lanes are summed through
// unrolled constant indices only (registers, no scratch).
template <int S>
__global__ __launch_bounds__(256) void k_ba_nodes(BoundApplyDev a, BoundNodesReqDev o) {
  constexpr int L = 4 + S;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (k >= a.n) return;
  const uint32_t nd = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.dcnt[k]), ni = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.icnt[k]);
  if (nd == 0u && ni == 0u) return;
  int64_t acc[L];                                          // inserts minus removes, this lane's share
#pragma unroll
  for (int l = 0; l < L; ++l) acc[l] = 0;
  uint32_t bits = 0;
  if (nd) {
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[k]), b1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.boff[k + 1]);
    for (uint32_t base = b0; base < b1; base += 64u) {
      const uint32_t j = base + lane;
      if (j < b1 && ((a.deadw[j >> 5] >> (j & 31u)) & 1u)) {
        bits |= a.bpres[j];
#pragma unroll
        for (int l = 0; l < L; ++l) acc[l] = wsub(acc[l], a.breq[(size_t)l * a.bstride + j]);
      }
    }
  }
  if (ni) {
    const uint32_t i0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ifirst[k]);
    for (uint32_t w = lane; w < ni; w += 64u) {
      const uint32_t src = i0 + w;
      bits |= a.ipres[src];
#pragma unroll
      for (int l = 0; l < L; ++l) acc[l] = wadd(acc[l], a.ireq[(size_t)l * a.n_insert + src]);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bits |= (uint32_t)__shfl_xor((int)bits, off);
#pragma unroll
    for (int l = 0; l < L; ++l) acc[l] = wadd(acc[l], (int64_t)__shfl_xor((long long)acc[l], off));
  }
  if (lane != 0) return;
  const uint32_t smask = S > 0 ? (uint32_t)((1ull << S) - 1ull) : 0u;
  const uint32_t rp = o.rpres[k], touched = bits & smask;
  bs_node_request r;
  r.index = k;
  r.requested_present = rp | touched;
#pragma unroll
  for (int l = 0; l < BS_MAX_LANES; ++l) r.requested[l] = 0;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int64_t raw = o.nreq[(size_t)l * o.nstride + k];
    const bool lane_on = l < 4 || ((touched >> (l - 4)) & 1u);
    if (!lane_on) { r.requested[l] = raw; continue; }
    const int64_t base = (l < 4 || ((rp >> (l - 4)) & 1u)) ? raw : 0;
    r.requested[l] = wadd(base, acc[l]);
  }
  const uint32_t slot = atomicAdd(o.count, 1u);
  if (slot < o.cap) o.out[slot] = r;
}

}  // namespace bs
