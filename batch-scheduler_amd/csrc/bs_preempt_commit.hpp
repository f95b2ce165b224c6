// bs_preempt_commit.hpp — preemption plans answered in sequence, and applied into the resident state (include/bsched.h,
// bs_preempt_commit).  Slot s (priority-descending, stable) sees the state after every earlier slot that got a node: its victims gone
// from the bound table and from their node's requests, itself added to its node as a nominated pod.
//
// Two launches for the plan, three more for BS_PREEMPT_APPLY (plain stores and launch boundaries only, no in-launch hand-over between
// workgroups):
//   k_pc_scan<S>     bs_preempt_run's scan (k_preempt_scan) against the BASE state, keeping the best kPcK pick keys of each
//                    (slot, node chunk) record in key order, plus the chunk's candidate count.
//   k_pc_resolve<S>  ONE persistent workgroup walks the slots in order.  Working state: per node the victims' requests removed so far
//                    (dv) and the nominees' requests added (dn) with their key bits, a dead flag per bound-table position, the dirty
//                    nodes (touched by an earlier slot).  For slot s: a clean chunk contributes its best record entry that is not
//                    dirty (exact: nodes outside a chunk's top kPcK are worse than all of them, and clean nodes' keys are unchanged);
//                    a chunk whose recorded entries are all dirty and that had more candidates than kPcK is rescanned (clean nodes,
//                    one per thread); every dirty node is re-evaluated on the working state (one per thread), and its candidacy on
//                    the base state is taken back out of the records' count.  Then the pick (block reduction), the victim list by
//                    wave 0 as k_preempt_pick writes it (64 bound pods per step, decisions replayed from broadcast lanes), the commit
//                    into the working state.  Three barriers per slot; the working state lives in global memory and is only read
//                    after a barrier by waves of the same workgroup (workgroup scope: same CU).
//   k_pc_nodes<S>    APPLY: the dirty nodes' new absolute request vectors (bs_node_request records) for k_nodes_assume.
//   k_pc_boff<S>     APPLY: survivors per node (boff length minus the victims counted in dv's pods lane), exclusive scan: new CSR.
//   k_pc_compact<S>  APPLY: one wave per node, a stable ballot compaction of every column into the new table.
// PDB bits (bpdb, bnviol; include/bsched.h, bs_bound_pdb_set) are fixed for the whole call.  The records are ordered by pre_better with the
// violation count in front, so the clean-chunk argument above holds for the widened key as it did for the old one; pc_eval and the victim
// list use bs_preempt.hpp's two-pass reprieve; k_pc_compact carries the column and recounts bnviol for the survivors.
// S is a template parameter for every scalar-lane count: register arrays are indexed by unrolled constants only (no scratch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_preempt.hpp"

namespace bs {

constexpr int kPcK = 4;              // pick keys kept per (slot, chunk) record
// the resolve's workgroup: 8 waves, 2 per SIMD (256 VGPRs a lane); 4 waves at 12 scalar lanes, whose registers need more (no scratch)
template <int S>
constexpr int pc_threads() { return S >= 12 ? 256 : 512; }

struct CommitDev {
  // bound table as loaded (CSR by node, importance order), plus the scalar keys of each entry
  const uint32_t* boff;
  const int32_t* bprio;
  const int64_t* bstart;
  const int32_t* bgroup;
  const int64_t* breq;      // [L][bstride]
  const uint32_t* bid;
  const uint32_t* bpres;
  const uint8_t* bpdb;      // [b] PDB-violating bit (bs_bound_pdb_set): fixed for the whole call, whatever earlier slots evict
  const uint32_t* bnviol;   // [n] entries of the node with the bit in the table as loaded (dead ones included: a shortcut only)
  uint32_t bstride;
  // this call: slots in priority-descending order (stable)
  uint32_t q, nchunks, chunk_nodes, cap;
  const uint32_t* spod;
  const int32_t* sprio;
  const uint32_t* sorig;
  const uint8_t* gprot;
  // records [nchunks][q][kPcK] (node -1 ends a record) and [nchunks][q] candidate counts
  int32_t* r_node;
  uint32_t* r_nv;
  uint32_t* r_npv;
  int32_t* r_top;
  int64_t* r_sum;
  int64_t* r_est;
  uint32_t* r_ncand;
  // working state (zeroed before the resolve)
  int64_t* dv;              // [L][n] requests of the victims taken off the node (pods lane: their count)
  int64_t* dn;              // [L][n] requests of the nominees added to the node (scalar lanes: present keys only)
  uint32_t* vbits;          // [n] scalar keys some victim of the node has
  uint32_t* nbits;          // [n] scalar keys some nominee of the node has
  uint8_t* dirty;           // [n]
  uint8_t* dead;            // [bstride]
  uint32_t* dlist;          // [q] dirty nodes, first touch order
  uint32_t* info;           // [2] dirty node count, victims in all
  // results in the caller's order
  int32_t* o_node;
  uint32_t* o_ncand;
  uint32_t* o_nv;
  uint32_t* o_npv;
  int32_t* o_top;
  int64_t* o_sum;
  int64_t* o_est;
  uint32_t* o_victims;      // [q][cap]
  const NomView* nm;        // the nominated-pod table (rule N), null without rows; static within the call
};

// APPLY: the compacted table (a second allocation; the old one is CommitDev's)
struct CompactDev {
  uint32_t* boff;
  int32_t* bprio;
  int64_t* bstart;
  int32_t* bgroup;
  int64_t* breq;
  uint32_t* bid;
  uint32_t* bpres;
  uint8_t* bpdb;
  uint32_t* bnviol;
  uint32_t bstride;
};

// the working state is rewritten inside k_pc_resolve: read it with vector loads (never the scalar cache), ordered by the barriers
__device__ __forceinline__ uint32_t pc_ld8(const uint8_t* p) { return (uint32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t pc_ld32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int64_t pc_ld64(const int64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// insert kk into the sorted list top[0..K) (best first), dropping the worst; unrolled: no dynamic register index
__device__ __forceinline__ void pc_insert(PreKey (&top)[kPcK], PreKey kk) {
#pragma unroll
  for (int i = 0; i < kPcK; ++i) {
    if (pre_better(kk, top[i])) {
      const PreKey t = top[i];
      top[i] = kk;
      kk = t;
    }
  }
}

template <int S>
__global__ __launch_bounds__(64) void k_pc_scan(NodesDev nd, PodsDev pd, CommitDev pe) {
  constexpr int L = 4 + S;
  const uint32_t tile = blockIdx.x, chunk = blockIdx.y, slot = tile * 64u + threadIdx.x;
  const bool valid = slot < pe.q;
  const uint32_t sl = valid ? slot : tile * 64u;
  const uint32_t pi = pe.spod[sl];
  const int32_t P = pe.sprio[sl];
  const int32_t pmax = pe.sprio[tile * 64u];
  int64_t rq[L];
  uint32_t rpq;
  pre_pod<S>(pd, pi, rq, rpq);
  const uint32_t cls = pd.cls[pi];
  const int32_t qg = pd.group[pi];
  const bool q_grouped = qg != BS_POD_NOT_GROUPED;
  const uint32_t k0 = chunk * pe.chunk_nodes, k1 = min(nd.n, k0 + pe.chunk_nodes);
  PreKey top[kPcK];
#pragma unroll
  for (int i = 0; i < kPcK; ++i) top[i] = pre_none();
  uint32_t ncand = 0;
  for (uint32_t k = k0; k < k1; ++k) {
    if (nd.flags[k]) continue;
    if (!valid || cls >= nd.n_classes || !((nd.fit[(size_t)cls * nd.fit_words + (k >> 5)] >> (k & 31u)) & 1u)) continue;
    const uint32_t b1 = pe.boff[k + 1];
    const uint32_t js = pre_below(pe.bprio, pe.boff[k], b1, pmax);
    int64_t al[L], cur[L];
    uint32_t apres;
    pre_node<S>(nd, k, al, cur, apres);
    pre_nominees<S>(pe.nm, k, P, cur);                                // rule N
    bool refused = false;
    for (uint32_t j = js; j < b1; ++j) {
      const int32_t pj = pe.bprio[j];
      if (pj >= P) continue;
      const int32_t vg = pe.bgroup[j];
      refused |= vg == BS_POD_NOT_GROUPED ? q_grouped : (vg < 0 || pe.gprot[vg] != 0 || (q_grouped && vg == qg));
#pragma unroll
      for (int l = 0; l < L; ++l) cur[l] = wsub(cur[l], pe.breq[(size_t)l * pe.bstride + j]);
    }
    if (refused || !pre_holds<S>(cur, al, apres, rq, rpq)) continue;
    ++ncand;
    if (top[kPcK - 1].node >= 0 && top[kPcK - 1].nv == 0) continue;   // kPcK nodes without victims: nothing later in the chunk enters
    // (kPcK victim-free nodes fill the record whatever violation counts later nodes have: a victim-free node wins outright)
    PreKey kk{(int32_t)k, 0u, 0u, 0, 0, 0};
    pre_reprieve<S>(pe, js, b1, P, pe.bnviol[k] != 0, nullptr, cur, al, apres, rq, rpq, kk);
    pc_insert(top, kk);
  }
  if (valid) {
    const size_t r = (size_t)chunk * pe.q + slot;
#pragma unroll
    for (int i = 0; i < kPcK; ++i) {
      pe.r_node[r * kPcK + i] = top[i].node;
      pe.r_nv[r * kPcK + i] = top[i].nv;
      pe.r_npv[r * kPcK + i] = top[i].npv;
      pe.r_top[r * kPcK + i] = top[i].top;
      pe.r_sum[r * kPcK + i] = top[i].sum;
      pe.r_est[r * kPcK + i] = top[i].est;
    }
    pe.r_ncand[r] = ncand;
  }
}

// one node against the working state for the slot (P, rq, rpq, cls, group): returns its pick key (node -1: no candidate); for a dirty
// node, *dcand gets its candidacy on the working state minus its candidacy on the base state (what the records counted)
template <int S>
__device__ bool pc_eval(const NodesDev& nd, const CommitDev& pe, uint32_t k, int32_t P, const int64_t (&rq)[4 + S], uint32_t rpq, uint32_t cls,
                        int32_t qg, bool dirty, PreKey& key, int32_t& dcand) {
  constexpr int L = 4 + S;
  key = pre_none();
  if (nd.flags[k]) return false;
  if (cls >= nd.n_classes || !((nd.fit[(size_t)cls * nd.fit_words + (k >> 5)] >> (k & 31u)) & 1u)) return false;
  const bool q_grouped = qg != BS_POD_NOT_GROUPED;
  const uint32_t b1 = pe.boff[k + 1];
  const uint32_t js = pre_below(pe.bprio, pe.boff[k], b1, P);   // [js, b1): the potential victims (the dead among them on dirty nodes)
  int64_t al[L], cur[L];
  uint32_t apres;
  if (dirty) {                                                   // the base state's answer, as the records counted it
    pre_node<S>(nd, k, al, cur, apres);
    pre_nominees<S>(pe.nm, k, P, cur);                          // rule N: the scan counted the rows too
    bool refused = false;
    for (uint32_t j = js; j < b1; ++j) {
      const int32_t vg = pe.bgroup[j];
      refused |= vg == BS_POD_NOT_GROUPED ? q_grouped : (vg < 0 || pe.gprot[vg] != 0 || (q_grouped && vg == qg));
#pragma unroll
      for (int l = 0; l < L; ++l) cur[l] = wsub(cur[l], pe.breq[(size_t)l * pe.bstride + j]);
    }
    if (!refused && pre_holds<S>(cur, al, apres, rq, rpq)) dcand -= 1;
  }
  pre_node<S>(nd, k, al, cur, apres);
  pre_nominees<S>(pe.nm, k, P, cur);                            // rule N (local: dv / dn never hold the rows)
  if (dirty) {
#pragma unroll
    for (int l = 0; l < L; ++l) cur[l] = wadd(wsub(cur[l], pc_ld64(pe.dv + (size_t)l * nd.n + k)), pc_ld64(pe.dn + (size_t)l * nd.n + k));
  }
  bool refused = false;
  for (uint32_t j = js; j < b1; ++j) {
    if (dirty && pc_ld8(pe.dead + j)) continue;
    const int32_t vg = pe.bgroup[j];
    refused |= vg == BS_POD_NOT_GROUPED ? q_grouped : (vg < 0 || pe.gprot[vg] != 0 || (q_grouped && vg == qg));
#pragma unroll
    for (int l = 0; l < L; ++l) cur[l] = wsub(cur[l], pe.breq[(size_t)l * pe.bstride + j]);
  }
  if (refused || !pre_holds<S>(cur, al, apres, rq, rpq)) return false;
  if (dirty) dcand += 1;
  key.node = (int32_t)k;
  pre_reprieve<S>(pe, js, b1, P, pe.bnviol[k] != 0, dirty ? pe.dead : nullptr, cur, al, apres, rq, rpq, key);
  return true;
}

__device__ __forceinline__ PreKey pc_shfl(const PreKey& a, int off) {
  PreKey b;
  b.node = __shfl_xor(a.node, off, 64);
  b.nv = (uint32_t)__shfl_xor((int)a.nv, off, 64);
  b.npv = (uint32_t)__shfl_xor((int)a.npv, off, 64);
  b.top = __shfl_xor(a.top, off, 64);
  b.sum = (int64_t)__shfl_xor((long long)a.sum, off, 64);
  b.est = (int64_t)__shfl_xor((long long)a.est, off, 64);
  return b;
}

template <int S>
__global__ __launch_bounds__(pc_threads<S>()) void k_pc_resolve(NodesDev nd, PodsDev pd, CommitDev pe) {
  constexpr int L = 4 + S;
  constexpr int kPcThreads = pc_threads<S>();
  constexpr int kWaves = kPcThreads / 64;
  __shared__ uint32_t s_res[kPcThreads];        // chunks to rescan this slot (at most nchunks; capped below by the walk)
  __shared__ uint32_t s_nres, s_ndirty, s_nvall;
  __shared__ PreKey s_key[kWaves];
  __shared__ int32_t s_dc[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t N = nd.n;
  if (t == 0) { s_nres = 0; s_ndirty = 0; s_nvall = 0; }
  __syncthreads();
  for (uint32_t s = 0; s < pe.q; ++s) {
    const uint32_t pi = pe.spod[s];
    const int32_t P = pe.sprio[s];
    int64_t rq[L];
    uint32_t rpq;
    pre_pod<S>(pd, pi, rq, rpq);
    const uint32_t cls = pd.cls[pi];
    const int32_t qg = pd.group[pi];
    // A: the records.  A chunk's best clean entry; a chunk with no clean entry among more than kPcK candidates goes to the rescan list
    PreKey best = pre_none();
    int32_t dc = 0;
    uint32_t pending = 0;                          // rescans this thread could not list (list full): done by this thread below
    for (uint32_t c = t; c < pe.nchunks; c += kPcThreads) {
      const size_t r = (size_t)c * pe.q + s;
      dc += (int32_t)pe.r_ncand[r];
      bool found = false;
#pragma unroll
      for (int i = 0; i < kPcK; ++i) {
        const int32_t node = pe.r_node[r * kPcK + i];
        if (!found && node >= 0 && !pc_ld8(pe.dirty + node)) {
          const PreKey kk{node, pe.r_nv[r * kPcK + i], pe.r_npv[r * kPcK + i], pe.r_top[r * kPcK + i], pe.r_sum[r * kPcK + i], pe.r_est[r * kPcK + i]};
          if (pre_better(kk, best)) best = kk;
          found = true;
        }
      }
      if (!found && pe.r_ncand[r] > (uint32_t)kPcK) {
        const uint32_t at = atomicAdd(&s_nres, 1u);
        if (at < (uint32_t)kPcThreads) s_res[at] = c;
        else ++pending;
      }
    }
    __syncthreads();
    // B: dirty nodes (working state), then the clean nodes of the rescanned chunks, one per thread
    const uint32_t nd_ = s_ndirty, nres = min(s_nres, (uint32_t)kPcThreads);
    const uint32_t items = nd_ + nres * pe.chunk_nodes;
    for (uint32_t i = t; i < items; i += kPcThreads) {
      uint32_t k;
      bool dirty;
      if (i < nd_) {
        k = pc_ld32(pe.dlist + i);
        dirty = true;
      } else {
        const uint32_t x = i - nd_, c = s_res[x / pe.chunk_nodes];
        k = c * pe.chunk_nodes + x % pe.chunk_nodes;
        if (k >= N || pc_ld8(pe.dirty + k)) continue;
        dirty = false;
      }
      PreKey kk;
      if (pc_eval<S>(nd, pe, k, P, rq, rpq, cls, qg, dirty, kk, dc) && pre_better(kk, best)) best = kk;
    }
    if (pending) {                                 // overflow of the rescan list (more than kPcThreads chunks): this thread's chunks
      for (uint32_t c = t; c < pe.nchunks; c += kPcThreads) {
        const size_t r = (size_t)c * pe.q + s;
        bool found = false;
#pragma unroll
        for (int i = 0; i < kPcK; ++i) {
          const int32_t node = pe.r_node[r * kPcK + i];
          found |= node >= 0 && !pc_ld8(pe.dirty + node);
        }
        if (found || pe.r_ncand[r] <= (uint32_t)kPcK) continue;
        bool listed = false;
        for (uint32_t x = 0; x < nres; ++x) listed |= s_res[x] == c;
        if (listed) continue;
        const uint32_t k0 = c * pe.chunk_nodes, k1 = min(N, k0 + pe.chunk_nodes);
        for (uint32_t k = k0; k < k1; ++k) {
          if (pc_ld8(pe.dirty + k)) continue;
          PreKey kk;
          if (pc_eval<S>(nd, pe, k, P, rq, rpq, cls, qg, false, kk, dc) && pre_better(kk, best)) best = kk;
        }
      }
    }
    // C: the pick
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const PreKey o = pc_shfl(best, off);
      if (pre_better(o, best)) best = o;
      dc += __shfl_xor(dc, off, 64);
    }
    if (lane == 0) { s_key[wave] = best; s_dc[wave] = dc; }
    __syncthreads();
    if (wave == 0) {
      best = lane < (uint32_t)kWaves ? s_key[lane] : pre_none();
      dc = lane < (uint32_t)kWaves ? s_dc[lane] : 0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const PreKey o = pc_shfl(best, off);
        if (pre_better(o, best)) best = o;
        dc += __shfl_xor(dc, off, 64);
      }
      const uint32_t orig = pe.sorig[s];
      const bool none = best.node < 0;
      if (lane == 0) {
        pe.o_node[orig] = best.node;
        pe.o_ncand[orig] = (uint32_t)dc;
        pe.o_nv[orig] = none ? 0u : best.nv;
        pe.o_npv[orig] = none ? 0u : best.npv;
        pe.o_top[orig] = none ? 0 : best.top;
        pe.o_sum[orig] = none ? 0 : best.sum;
        pe.o_est[orig] = none ? 0 : best.est;
      }
      if (!none) {
        // D: the victim list on the chosen node (working state), then the commit
        const uint32_t k = (uint32_t)best.node;
        int64_t al[L], cur[L];
        uint32_t apres;
        pre_node<S>(nd, k, al, cur, apres);
        // the node's working deltas: lane l loads lane l's word (a vector load: the words are rewritten inside this launch)
        int64_t mdv = 0, mdn = 0;
        if (lane < (uint32_t)L) { mdv = pc_ld64(pe.dv + (size_t)lane * N + k); mdn = pc_ld64(pe.dn + (size_t)lane * N + k); }
        const uint32_t mvb = pc_ld32(pe.vbits + k), mnb = pc_ld32(pe.nbits + k);
        const bool was_dirty = pc_ld8(pe.dirty + k) != 0;
        int64_t vsum[L];
#pragma unroll
        for (int l = 0; l < L; ++l) {
          cur[l] = wadd(wsub(cur[l], pre_readlane64(mdv, l)), pre_readlane64(mdn, l));
          vsum[l] = 0;
        }
        uint32_t vb = 0;
        const uint32_t b1 = pe.boff[k + 1];
        const uint32_t js = pre_below(pe.bprio, pe.boff[k], b1, P);
        int64_t part[L];
#pragma unroll
        for (int l = 0; l < L; ++l) part[l] = 0;
        for (uint32_t j = js + lane; j < b1; j += 64u) {
          if (pc_ld8(pe.dead + j)) continue;
#pragma unroll
          for (int l = 0; l < L; ++l) part[l] = wadd(part[l], pe.breq[(size_t)l * pe.bstride + j]);
        }
        pre_nominees_part<S>(pe.nm, k, P, lane, part);          // rule N
#pragma unroll
        for (int l = 0; l < L; ++l) {
          int64_t v = part[l];
          for (int off = 32; off > 0; off >>= 1) v = wadd(v, (int64_t)__shfl_xor((long long)v, off, 64));
          cur[l] = wsub(cur[l], v);
        }
        uint32_t nv = 0;
        uint32_t* vout = pe.o_victims + (size_t)orig * pe.cap;
        // two passes over the same windows where the node holds violating pods (the violating entries first): reprieve order
        const bool pdb = pe.bnviol[k] != 0;
        const uint32_t npass = pdb ? 2u : 1u;
        for (uint32_t pass = 0; pass < npass; ++pass) {
          for (uint32_t base = js; base < b1; base += 64u) {
            const uint32_t j = base + lane;
            const bool have = j < b1 && !pc_ld8(pe.dead + j) && (!pdb || (pe.bpdb[j] != 0) == (pass == 0));
            uint64_t live = __ballot(have);
            if (!live) continue;
            int64_t mine[L];
#pragma unroll
            for (int l = 0; l < L; ++l) mine[l] = have ? pe.breq[(size_t)l * pe.bstride + j] : 0;
            const uint32_t myid = have ? pe.bid[j] : 0u, mypres = have ? pe.bpres[j] : 0u;
            uint64_t vmask = 0;
            while (live) {
              const uint32_t i = (uint32_t)__builtin_ctzll(live);
              live &= live - 1;
              int64_t tt[L];
#pragma unroll
              for (int l = 0; l < L; ++l) tt[l] = wadd(cur[l], pre_readlane64(mine[l], i));
              if (pre_holds<S>(tt, al, apres, rq, rpq)) {
#pragma unroll
                for (int l = 0; l < L; ++l) cur[l] = tt[l];
              } else {
                const uint32_t vid = (uint32_t)__builtin_amdgcn_readlane((int)myid, (int)i);
                if (lane == 0 && nv < pe.cap) vout[nv] = vid;
                ++nv;
                vmask |= 1ull << i;
#pragma unroll
                for (int l = 0; l < L; ++l) vsum[l] = wadd(vsum[l], pre_readlane64(mine[l], i));
                vb |= (uint32_t)__builtin_amdgcn_readlane((int)mypres, (int)i);
              }
            }
            if ((vmask >> lane) & 1ull) pe.dead[j] = 1;
          }
        }
        // commit: the victims leave (RemovePod), the preemptor is nominated on the node (AddPod)
        const uint32_t smask = S > 0 ? (uint32_t)((1ull << S) - 1ull) : 0u;
        if (lane < (uint32_t)L) {
          int64_t add = 0, rem = 0;
#pragma unroll
          for (int l = 0; l < L; ++l) {
            if ((int)lane == l) {
              rem = vsum[l];
              add = l < 3 ? rq[l] : (l == 3 ? 1 : (((rpq >> (l - 4)) & 1u) ? rq[l] : 0));
            }
          }
          pe.dv[(size_t)lane * N + k] = wadd(mdv, rem);
          pe.dn[(size_t)lane * N + k] = wadd(mdn, add);
        }
        if (lane == 0) {
          pe.vbits[k] = mvb | (vb & smask);
          pe.nbits[k] = mnb | (rpq & smask);
          if (!was_dirty) {
            pe.dirty[k] = 1;
            pe.dlist[s_ndirty] = k;
            s_ndirty = s_ndirty + 1;
          }
          s_nvall = s_nvall + nv;
        }
      }
      if (lane == 0) s_nres = 0;
    }
    __syncthreads();
  }
  if (t == 0) { pe.info[0] = s_ndirty; pe.info[1] = s_nvall; }
}

// APPLY: node i of the dirty list gets base - victims (+ nominees with ASSUME); scalar lanes no victim / nominee has keep their word and
// their present bit, the others are set (an absent key counts as 0)
template <int S>
__global__ void k_pc_nodes(NodesDev nd, CommitDev pe, uint32_t ndirty, uint32_t assume, bs_node_request* out) {
  constexpr int L = 4 + S;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ndirty) return;
  const uint32_t k = pe.dlist[i], N = nd.n;
  const uint32_t rp = nd.rpres[k];
  const uint32_t touched = pe.vbits[k] | (assume ? pe.nbits[k] : 0u);
  bs_node_request r;
  r.index = k;
  r.requested_present = rp | touched;
#pragma unroll
  for (int l = 0; l < BS_MAX_LANES; ++l) r.requested[l] = 0;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int64_t raw = nd.req[(size_t)l * nd.stride + k];
    const bool lane_on = l < 4 || ((touched >> (l - 4)) & 1u);
    if (!lane_on) { r.requested[l] = raw; continue; }
    const int64_t base = (l < 4 || ((rp >> (l - 4)) & 1u)) ? raw : 0;
    int64_t v = wsub(base, pe.dv[(size_t)l * N + k]);
    if (assume) v = wadd(v, pe.dn[(size_t)l * N + k]);
    r.requested[l] = v;
  }
  out[i] = r;
}

// APPLY: the new CSR offsets, one block (survivors of node k = its length minus its victims, dv's pods lane)
template <int S>
__global__ __launch_bounds__(1024) void k_pc_boff(CommitDev pe, uint32_t n, uint32_t* nboff) {
  __shared__ uint32_t s_part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + 1023u) / 1024u, a = min(n, t * per), b = min(n, a + per);
  uint32_t sum = 0;
  for (uint32_t k = a; k < b; ++k) sum += (pe.boff[k + 1] - pe.boff[k]) - (uint32_t)pe.dv[(size_t)3 * n + k];
  s_part[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {       // inclusive scan (Hillis-Steele)
    const uint32_t v = t >= off ? s_part[t - off] : 0u;
    __syncthreads();
    s_part[t] += v;
    __syncthreads();
  }
  uint32_t run = t ? s_part[t - 1] : 0u;
  for (uint32_t k = a; k < b; ++k) {
    nboff[k] = run;
    run += (pe.boff[k + 1] - pe.boff[k]) - (uint32_t)pe.dv[(size_t)3 * n + k];
  }
  if (t == 1023u) nboff[n] = s_part[1023];
}

// APPLY: one wave per node, the survivors in table order (stable)
template <int S>
__global__ __launch_bounds__(64) void k_pc_compact(CommitDev pe, CompactDev nw, uint32_t n) {
  constexpr int L = 4 + S;
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  if (k >= n) return;
  const uint32_t b0 = pe.boff[k], b1 = pe.boff[k + 1];
  uint32_t dst = nw.boff[k];
  const bool any_dead = pe.dirty[k] != 0;
  uint32_t nviol = 0;
  for (uint32_t base = b0; base < b1; base += 64u) {
    const uint32_t j = base + lane;
    const bool keep = j < b1 && !(any_dead && pe.dead[j]);
    const uint8_t pdb = keep ? pe.bpdb[j] : (uint8_t)0;
    const uint64_t m = __ballot(keep);
    nviol += (uint32_t)__builtin_popcountll(__ballot(pdb != 0));
    const uint32_t rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (keep) {
      const uint32_t d = dst + rank;
      nw.bprio[d] = pe.bprio[j];
      nw.bstart[d] = pe.bstart[j];
      nw.bgroup[d] = pe.bgroup[j];
      nw.bid[d] = pe.bid[j];
      nw.bpres[d] = pe.bpres[j];
      nw.bpdb[d] = pdb;
#pragma unroll
      for (int l = 0; l < L; ++l) nw.breq[(size_t)l * nw.bstride + d] = pe.breq[(size_t)l * pe.bstride + j];
    }
    dst += (uint32_t)__builtin_popcountll(m);
  }
  if (lane == 0) nw.bnviol[k] = nviol;        // the survivors' count: a node whose violating pods all left is one-pass again
}

}  // namespace bs
