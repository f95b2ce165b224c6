// bs_bound_nodes.hpp — the resident bound-pod table follows node-list surgery (include/bsched.h, bs_bound_nodes_apply): the lists of
// removed nodes leave with their nodes, every later node moves down, appended nodes arrive empty.  The host reduces the delta list to the
// sorted OLD indices that leave and the count of appended nodes that stay (bs_bound_nodes_replay.hpp, O(count)); the device makes one pass
// over the table into the second allocation (as BS_PREEMPT_APPLY and bs_bound_apply do), which the host swaps in after it read the dropped
// count back.  No list changes inside: every surviving node is a straight copy.
//
// Four launches (plain loads and stores, no atomics; hand-over between kernels by launch boundaries only):
//   k_bn_len<S>    one thread per NEW node k': its old node is k' + j for the first j with rem[j] - j > k' (a binary search of the removed
//                  list; an appended node has none): len[k'] and src[k'] = the old list's start (kBnNone for none).  One thread per
//                  REMOVED node: dlen[t] = its list's length.
//   k_bn_scan1<S>  exclusive scans, 1024 entries per block, each block on its own: blockIdx.y = 0 scans len into the new CSR (nw.boff),
//                  blockIdx.y = 1 scans dlen into doff (where each removed node's ids go in dropped_ids: old-table order).  The block
//                  totals go to bsum.
//   k_bn_scan2<S>  every block adds the totals of the blocks in front of it; the last one writes the grand total behind the scan
//                  (nw.boff[n1] = the new entry count, doff[nrem] = the dropped count) and into the word pair the host reads.
//                  (k_pc_boff / k_ba_boff scan the same lengths in ONE block, 48 us at 20 000 nodes: this pair is the form they could take.)
//   k_bn_move<S>   one wave per new node, four per workgroup: every column of src[k'] .. + len into the new offset, 64 entries per step,
//                  one entry per lane (a list starts anywhere inside a column and holds tens of entries: 4- and 8-byte accesses, coalesced
//                  across the wave; nothing here is 16-byte aligned).  Lane 0 writes the node's PDB count; an appended node writes a zero
//                  count only.  Behind the new nodes one wave per REMOVED node copies its ids to dropped[doff[t] ..], cut at the cap.
// The new table's column offsets depend on its entry count, which only the scan knows: k_bn_move computes them from nw.boff[n1] with the
// function the host uses (bound_layout, bs_kernels.hpp), in an allocation the host sized for the OLD entry count (the count cannot grow here).
// S is a template parameter as for every kernel of this code object; the request lanes move through an unrolled loop, load to store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_kernels.hpp"

namespace bs {

constexpr uint32_t kBnNone = 0xffffffffu;

struct BoundNodesDev {
  // the live table (read only here)
  const uint32_t* boff;
  const int32_t* bprio;
  const int64_t* bstart;
  const int32_t* bgroup;
  const int64_t* breq;      // [L][bstride]
  const uint32_t* bid;
  const uint32_t* bpres;
  const uint8_t* bpdb;
  uint32_t bstride, n0, n1; // old lane stride; node counts before and after
  // the delta
  uint32_t nrem, old_left;  // removed old nodes; n0 - nrem: new nodes below it have an old node, the others are appended
  const uint32_t* rem;      // [nrem] old indices, ascending
  // the new table: its allocation (the CSR sits at offset 0 whatever the entry count is)
  uint8_t* nbase;
  uint32_t* nboff;          // [n1 + 1]
  // scratch of this call
  uint32_t* len;            // [n1]
  uint32_t* src;            // [n1]
  uint32_t* dlen;           // [nrem]
  uint32_t* doff;           // [nrem + 1]
  uint32_t* bsum;           // [2][nblk] block totals of the two scans
  uint32_t nblk;            // max(1, ceil(max(n1, nrem) / 1024))
  uint32_t* pair;           // {new entry count, dropped count}
  uint32_t* dropped;        // [min(dropped_cap, old entry count)]
  uint32_t dropped_cap;
};

template <int S>
__global__ __launch_bounds__(256) void k_bn_len(BoundNodesDev a) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t < a.n1) {
    uint32_t len = 0, src = kBnNone;
    if (t < a.old_left) {
      uint32_t lo = 0, hi = a.nrem;                          // the first j with rem[j] - j > t: j removed nodes sit in front of the old node
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.rem[mid] - mid <= t) lo = mid + 1u;
        else hi = mid;
      }
      const uint32_t old = t + lo;                           // < n0: old_left = n0 - nrem
      src = a.boff[old];
      len = a.boff[old + 1] - src;
    }
    a.len[t] = len;
    a.src[t] = src;
  }
  if (t < a.nrem) {
    const uint32_t r = a.rem[t];
    a.dlen[t] = a.boff[r + 1] - a.boff[r];
  }
}

// the two scans' operands by blockIdx.y
template <int S>
__device__ __forceinline__ void bn_scan_job(const BoundNodesDev& a, const uint32_t*& in, uint32_t*& out, uint32_t& n) {
  if (blockIdx.y == 0) { in = a.len; out = a.nboff; n = a.n1; }
  else { in = a.dlen; out = a.doff; n = a.nrem; }
}

template <int S>
__global__ __launch_bounds__(1024) void k_bn_scan1(BoundNodesDev a) {
  __shared__ uint32_t s_part[1024];
  const uint32_t* in;
  uint32_t* out;
  uint32_t n;
  bn_scan_job<S>(a, in, out, n);
  const uint32_t t = threadIdx.x, i = blockIdx.x * 1024u + t;
  const uint32_t v = i < n ? in[i] : 0u;
  s_part[t] = v;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {           // inclusive scan (Hillis-Steele, as k_ba_boff)
    const uint32_t w = t >= off ? s_part[t - off] : 0u;
    __syncthreads();
    s_part[t] += w;
    __syncthreads();
  }
  if (i < n) out[i] = s_part[t] - v;
  if (t == 1023u) a.bsum[blockIdx.y * a.nblk + blockIdx.x] = s_part[1023];
}

template <int S>
__global__ __launch_bounds__(1024) void k_bn_scan2(BoundNodesDev a) {
  __shared__ uint32_t s_part[1024];
  const uint32_t* in;
  uint32_t* out;
  uint32_t n;
  bn_scan_job<S>(a, in, out, n);
  const uint32_t t = threadIdx.x, blk = blockIdx.x;
  const uint32_t* bsum = a.bsum + blockIdx.y * a.nblk;
  uint32_t part = 0;
  for (uint32_t x = t; x < blk; x += 1024u) part += bsum[x];
  s_part[t] = part;
  __syncthreads();
  for (uint32_t off = 512u; off; off >>= 1) {
    if (t < off) s_part[t] += s_part[t + off];
    __syncthreads();
  }
  const uint32_t pre = s_part[0], i = blk * 1024u + t;
  if (i < n) out[i] += pre;
  if (blk == a.nblk - 1u && t == 0) {                        // (blocks behind a scan's last entry hold zero totals)
    const uint32_t total = pre + bsum[blk];
    out[n] = total;
    a.pair[blockIdx.y] = total;
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_bn_move(BoundNodesDev a) {
  constexpr int L = 4 + S;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (w >= a.n1) {                                           // the ids of a removed node's list, in the old table's order
    const uint32_t t = w - a.n1;
    if (t >= a.nrem || a.dropped_cap == 0u) return;
    const uint32_t r = a.rem[t], b0 = a.boff[r], len = a.boff[r + 1] - b0, d0 = a.doff[t];
    for (uint32_t x = lane; x < len && d0 + x < a.dropped_cap; x += 64u) a.dropped[d0 + x] = a.bid[b0 + x];
    return;
  }
  const uint32_t b2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.nboff[a.n1]);
  BoundLayout lay;
  bound_layout((uint32_t)L, a.n1, b2, lay);
  uint32_t* nviol = reinterpret_cast<uint32_t*>(a.nbase + lay.nviol);
  const uint32_t src = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.src[w]);
  if (src == kBnNone) {
    if (lane == 0) nviol[w] = 0u;
    return;
  }
  int32_t* nprio = reinterpret_cast<int32_t*>(a.nbase + lay.prio);
  int64_t* nstart = reinterpret_cast<int64_t*>(a.nbase + lay.start);
  int32_t* ngroup = reinterpret_cast<int32_t*>(a.nbase + lay.group);
  uint32_t* nid = reinterpret_cast<uint32_t*>(a.nbase + lay.id);
  int64_t* nreq = reinterpret_cast<int64_t*>(a.nbase + lay.req);
  uint32_t* npres = reinterpret_cast<uint32_t*>(a.nbase + lay.pres);
  uint8_t* npdb = a.nbase + lay.pdb;
  const size_t nstride = b2 ? b2 : 1u;
  const uint32_t len = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.len[w]);
  const uint32_t dst = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.nboff[w]);
  uint32_t viol = 0;
  for (uint32_t base = 0; base < len; base += 64u) {
    const uint32_t x = base + lane;
    const bool in = x < len;
    const uint32_t j = src + x, d = dst + x;
    const uint8_t pdb = in ? a.bpdb[j] : (uint8_t)0;
    viol += (uint32_t)__builtin_popcountll(__ballot(pdb != 0));
    if (in) {
      nprio[d] = a.bprio[j];
      nstart[d] = a.bstart[j];
      ngroup[d] = a.bgroup[j];
      nid[d] = a.bid[j];
      npres[d] = a.bpres[j];
      npdb[d] = pdb;
#pragma unroll
      for (int l = 0; l < L; ++l) nreq[(size_t)l * nstride + d] = a.breq[(size_t)l * a.bstride + j];
    }
  }
  if (lane == 0) nviol[w] = viol;
}

}  // namespace bs
