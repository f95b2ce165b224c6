// bs_preempt.hpp — gang-aware preemption: the victim search upstream's generic_scheduler.go runs for a pod that passed PreFilter and
// found no node (selectVictimsOnNode on every node, with the plugin's PreemptRemovePod, core.go:197-260, gating every removal; then
// pickOneNodeForPreemption), for a whole batch of preemptors at once.  Semantics and restrictions: include/bsched.h, bs_preempt_run.
//
// Two launches with a launch boundary between them (plain stores, no in-launch hand-over):
//   k_preempt_scan<S>  grid (tile of 64 preemptors, chunk of nodes), one wave per block.  Lane = preemptor; the preemptors are sorted by
//                      priority (descending) on the host, so a tile's potential victims on a node are all inside the suffix of the node's
//                      list that lies below the tile's highest priority, and the node's bound pods are wave-uniform data (broadcast
//                      loads).  Each lane keeps its running node requests in VGPRs, walks the suffix twice (remove-all + policy, then
//                      the reprieve) and keeps its best pick key over the chunk in registers; one record per (preemptor, chunk).
//                      On a node that holds a PDB-violating pod (bnviol[k] != 0, wave-uniform) the reprieve is two predicated passes
//                      over the suffix: the violating entries first, then the others (pre_reprieve).
//   k_preempt_pick<S>  one wave per preemptor: reduces the chunk records (lowest node index wins every tie: records hold node indices,
//                      and the key ends in the node index), then recomputes the reprieve on the winning node to write the victim list —
//                      64 bound pods are loaded at a time, one per lane, and every lane replays the same sequential decision from
//                      broadcast lanes (v_readlane), so the walk costs no dependent memory trip per pod.  With violating pods on
//                      the node the same 64-entry windows are replayed twice, violating entries first: the list is in reprieve order.
// S is a template parameter for EVERY scalar-lane count up to BS_MAX_SCALARS: the request vectors are register arrays indexed by
// unrolled constants only (no scratch in any instantiation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_kernels.hpp"
#include "bs_nom_view.hpp"

namespace bs {

__device__ __forceinline__ int64_t pre_readlane64(int64_t v, uint32_t i) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)i);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), (int)i);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// (NomView, the resident nominated-pod table as the victim search reads it, and kNmNone: bs_nom_view.hpp, shared with the sequential pass)

// Rule N (include/bsched.h): the rows on node k with priority >= P are added into the LOCAL cur (wrapping sums; the order of a chain does
// not matter).  The sum is never stored: the working deltas of a plan, k_pc_nodes' vectors, the gang rollback and the host mirror do not
// see it.  In the scan kernels k is wave-uniform and P is the lane's.  Without rows: one uniform branch.
template <int S>
__device__ __forceinline__ void pre_nominees(const NomView* view, uint32_t k, int32_t P, int64_t (&cur)[4 + S]) {
  if (!view) return;
  const NomView nm = *view;
  for (uint32_t r = nm.nhead[k]; r != kNmNone; r = nm.nnext[r]) {
    if (nm.nprio[r] < P) continue;
#pragma unroll
    for (int l = 0; l < 4 + S; ++l) cur[l] = wadd(cur[l], nm.nreq[(size_t)l * nm.nstride + r]);
  }
}

// ... where a whole wave works on one node for one preemptor (k and P wave-uniform: k_preempt_pick, stage D of the resolve kernels) and is
// about to reduce part[] = the potential victims' requests, which it SUBTRACTS from cur: lane l < L loads request lane l of each
// qualifying row (one load a row) and takes it off its own part[l] (wrapping sums: cur - (victims - rows) = cur - victims + rows,
// exactly).  The walk rides the reduction that is there: one register pair of its own, no broadcast.
template <int S>
__device__ __forceinline__ void pre_nominees_part(const NomView* view, uint32_t k, int32_t P, uint32_t lane, int64_t (&part)[4 + S]) {
  if (!view) return;
  const NomView nm = *view;
  for (uint32_t r = nm.nhead[k]; r != kNmNone; r = nm.nnext[r]) {
    if (nm.nprio[r] < P) continue;
    const int64_t v = lane < (uint32_t)(4 + S) ? nm.nreq[(size_t)lane * nm.nstride + r] : 0;
#pragma unroll
    for (int l = 0; l < 4 + S; ++l) part[l] = wsub(part[l], (int)lane == l ? v : 0);
  }
}

// what both launches read (device pointers; the bound table is resident, the rest belongs to one bs_preempt_run)
struct PreemptDev {
  // bound table, CSR by node, importance order within a node (priority descending, start ascending, caller id ascending)
  const uint32_t* boff;     // [n + 1]
  const int32_t* bprio;     // [b]
  const int64_t* bstart;    // [b]
  const int32_t* bgroup;    // [b] group index, BS_POD_NOT_GROUPED or BS_POD_GROUP_MISSING
  const int64_t* breq;      // [L][bstride]: lanes 0..2 as loaded, lane 3 = 1 (one pod), scalar lanes 0 where the key is absent
  const uint32_t* bid;      // [b] caller's numbering
  const uint8_t* bpdb;      // [b] evicting the pod would violate a PodDisruptionBudget (bs_bound_pdb_set)
  const uint32_t* bnviol;   // [n] entries of the node with that bit: 0 = the node takes the one-pass reprieve
  uint32_t bstride;
  // this call: preemptor slots in priority-descending order
  uint32_t q, nchunks, chunk_nodes, cap;
  const uint32_t* spod;     // [q] resident-queue index
  const int32_t* sprio;     // [q]
  const uint32_t* sorig;    // [q] position in the caller's arrays
  const uint8_t* gprot;     // [g] group is Scheduled / Running
  // chunk records, [nchunks][q]
  int32_t* r_node;
  uint32_t* r_nv;
  uint32_t* r_npv;
  int32_t* r_top;
  int64_t* r_sum;
  int64_t* r_est;
  uint32_t* r_ncand;
  // results in the caller's order
  int32_t* o_node;
  uint32_t* o_ncand;
  uint32_t* o_nv;
  uint32_t* o_npv;          // PDB-violating victims (bs_preempt_pdb_read)
  int32_t* o_top;
  int64_t* o_sum;
  int64_t* o_est;
  uint32_t* o_victims;      // [q][cap]
  const NomView* nm;        // the nominated-pod table (rule N), null without rows
};

// pick key of one candidate node (pickOneNodeForPreemption): node < 0 = no candidate
// top = priority of the FIRST LISTED victim (upstream reads victims.Pods[0]); est = earliest start among the victims of the true
// maximum priority (GetEarliestPodStartTime walks every victim): with a violating victim in front the two look at different priorities
struct PreKey {
  int32_t node;
  uint32_t nv;
  uint32_t npv;             // victims that came from the violating list
  int32_t top;
  int64_t sum;
  int64_t est;
};
__device__ __forceinline__ PreKey pre_none() { return PreKey{-1, 0u, 0u, 0, 0, 0}; }

// a strictly better than b: a node without victims wins outright (lowest index among several); otherwise the lexicographically
// smallest (PDB violations, first listed victim's priority, sum of priority + 2^31, victim count, -earliest start of the
// top-priority victims, node index)
__device__ __forceinline__ bool pre_better(const PreKey& a, const PreKey& b) {
  if (a.node < 0) return false;
  if (b.node < 0) return true;
  if (a.nv == 0 || b.nv == 0) return (a.nv == 0 && b.nv == 0) ? a.node < b.node : a.nv == 0;
  if (a.npv != b.npv) return a.npv < b.npv;
  if (a.top != b.top) return a.top < b.top;
  if (a.sum != b.sum) return a.sum < b.sum;
  if (a.nv != b.nv) return a.nv < b.nv;
  if (a.est != b.est) return a.est > b.est;
  return a.node < b.node;
}

// bs_seq_run's first-fit rule (include/bsched.h, bs_seq_run) against the requests `cur` (scalar lanes: the effective value, 0 where the
// node had no key): cpu / mem / eph bind when the pod asks for them, pods lane requested + 1 <= allocatable, a requested scalar needs
// the allocatable key
template <int S>
__device__ __forceinline__ bool pre_holds(const int64_t (&cur)[4 + S], const int64_t (&al)[4 + S], uint32_t apres, const int64_t (&rq)[4 + S],
                                          uint32_t rpq) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) ok &= !(rq[j] > 0 && rq[j] > wsub(al[j], cur[j]));
  ok &= !(wadd(cur[3], 1) > al[3]);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (((rpq >> s) & 1u) && rq[4 + s] > 0) ok &= ((apres >> s) & 1u) && !(rq[4 + s] > wsub(al[4 + s], cur[4 + s]));
  }
  return ok;
}

// first entry of [b0, b1) whose priority is below p (the list is in priority-descending order); uniform
__device__ __forceinline__ uint32_t pre_below(const int32_t* prio, uint32_t b0, uint32_t b1, int32_t p) {
  while (b0 < b1) {
    const uint32_t mid = (b0 + b1) >> 1;
    if (prio[mid] < p) b1 = mid; else b0 = mid + 1;
  }
  return b0;
}

template <int S>
__device__ __forceinline__ void pre_node(const NodesDev& nd, uint32_t k, int64_t (&al)[4 + S], int64_t (&cur)[4 + S], uint32_t& apres) {
  apres = nd.apres[k];
  const uint32_t rp = nd.rpres[k];
#pragma unroll
  for (int l = 0; l < 4 + S; ++l) {
    al[l] = nd.alloc[(size_t)l * nd.stride + k];
    const int64_t r = nd.req[(size_t)l * nd.stride + k];
    cur[l] = (l < 4 || ((rp >> (l - 4)) & 1u)) ? r : 0;
  }
}

template <int S>
__device__ __forceinline__ void pre_pod(const PodsDev& pd, uint32_t pi, int64_t (&rq)[4 + S], uint32_t& rpq) {
#pragma unroll
  for (int l = 0; l < 4 + S; ++l) rq[l] = pd.req[(size_t)l * pd.p + pi];
  rpq = pd.pres[pi];
}

// step 5, the reprieve, on the entries [js, b1) of one node from the state `cur` with every potential victim (priority < P) removed;
// fills kk's victim fields.  pdb = the node holds a violating pod: the entries are offered in two predicated passes, the violating
// ones first (importance order inside a pass), as upstream's selectVictimsOnNode reprieves violatingVictims before
// nonViolatingVictims.  Inside a pass the first victim is the most important one; across the passes it is not, so est follows
// (mx = the true maximum victim priority, earliest start at mx) while top stays with the first listed victim.  Without pdb this is
// the single pass and the loads it always was.  dead != nullptr: entries an earlier slot evicted (bs_preempt_commit's working
// state, rewritten inside the launch: a vector load) are skipped.
template <int S, class D>
__device__ __forceinline__ void pre_reprieve(const D& pe, uint32_t js, uint32_t b1, int32_t P, bool pdb, const uint8_t* dead, int64_t (&cur)[4 + S],
                                             const int64_t (&al)[4 + S], uint32_t apres, const int64_t (&rq)[4 + S], uint32_t rpq, PreKey& kk) {
  constexpr int L = 4 + S;
  int32_t mx = 0;
  const uint32_t npass = pdb ? 2u : 1u;
  for (uint32_t pass = 0; pass < npass; ++pass) {
    for (uint32_t j = js; j < b1; ++j) {
      const int32_t pj = pe.bprio[j];
      if (pj >= P) continue;
      if (dead && __hip_atomic_load(dead + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
      if (pdb && (pe.bpdb[j] != 0) != (pass == 0)) continue;
      int64_t t[L];
#pragma unroll
      for (int l = 0; l < L; ++l) t[l] = wadd(cur[l], pe.breq[(size_t)l * pe.bstride + j]);
      if (pre_holds<S>(t, al, apres, rq, rpq)) {
#pragma unroll
        for (int l = 0; l < L; ++l) cur[l] = t[l];
      } else {
        if (kk.nv == 0) {
          kk.top = pj;
          mx = pj;
          kk.est = pe.bstart[j];
        } else if (pass && pj >= mx) {
          const int64_t st = pe.bstart[j];
          if (pj > mx || st < kk.est) { mx = pj; kk.est = st; }
        }
        ++kk.nv;
        kk.npv += (pdb && pass == 0) ? 1u : 0u;
        kk.sum += (int64_t)pj + 2147483648LL;
      }
    }
  }
}

template <int S>
__global__ __launch_bounds__(64) void k_preempt_scan(NodesDev nd, PodsDev pd, PreemptDev pe) {
  constexpr int L = 4 + S;
  const uint32_t tile = blockIdx.x, chunk = blockIdx.y, slot = tile * 64u + threadIdx.x;
  const bool valid = slot < pe.q;
  const uint32_t sl = valid ? slot : tile * 64u;
  const uint32_t pi = pe.spod[sl];
  const int32_t P = pe.sprio[sl];
  const int32_t pmax = pe.sprio[tile * 64u];            // slots are in priority-descending order: the tile's highest
  int64_t rq[L];
  uint32_t rpq;
  pre_pod<S>(pd, pi, rq, rpq);
  const uint32_t cls = pd.cls[pi];
  const int32_t qg = pd.group[pi];
  const bool q_grouped = qg != BS_POD_NOT_GROUPED;
  const uint32_t k0 = chunk * pe.chunk_nodes, k1 = min(nd.n, k0 + pe.chunk_nodes);
  PreKey best = pre_none();
  uint32_t ncand = 0;
  for (uint32_t k = k0; k < k1; ++k) {
    if (nd.flags[k]) continue;                                                       // step 1: flagged node
    if (!valid || cls >= nd.n_classes || !((nd.fit[(size_t)cls * nd.fit_words + (k >> 5)] >> (k & 31u)) & 1u)) continue;   // step 1: checkFit
    const uint32_t b1 = pe.boff[k + 1];
    const uint32_t js = pre_below(pe.bprio, pe.boff[k], b1, pmax);
    int64_t al[L], cur[L];
    uint32_t apres;
    pre_node<S>(nd, k, al, cur, apres);
    pre_nominees<S>(pe.nm, k, P, cur);                                                // rule N
    // steps 2-4: remove every potential victim (priority < P), each through the policy of PreemptRemovePod
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
    if (best.node >= 0 && best.nv == 0) continue;              // nothing later in the chunk beats a node without victims
    // step 5: reprieve in importance order, the violating entries first where the node has any.  (The early-out above stays valid
    // with PDBs: a node without victims still wins outright, whatever the others' violation counts.)
    PreKey kk{(int32_t)k, 0u, 0u, 0, 0, 0};
    pre_reprieve<S>(pe, js, b1, P, pe.bnviol[k] != 0, nullptr, cur, al, apres, rq, rpq, kk);
    if (pre_better(kk, best)) best = kk;
  }
  if (valid) {
    const size_t r = (size_t)chunk * pe.q + slot;
    pe.r_node[r] = best.node;
    pe.r_nv[r] = best.nv;
    pe.r_npv[r] = best.npv;
    pe.r_top[r] = best.top;
    pe.r_sum[r] = best.sum;
    pe.r_est[r] = best.est;
    pe.r_ncand[r] = ncand;
  }
}

template <int S>
__global__ __launch_bounds__(64) void k_preempt_pick(NodesDev nd, PodsDev pd, PreemptDev pe) {
  constexpr int L = 4 + S;
  __shared__ PreKey sk[64];
  __shared__ uint32_t sc[64];
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  PreKey best = pre_none();
  uint32_t ncand = 0;
  for (uint32_t c = lane; c < pe.nchunks; c += 64u) {
    const size_t r = (size_t)c * pe.q + slot;
    const PreKey kk{pe.r_node[r], pe.r_nv[r], pe.r_npv[r], pe.r_top[r], pe.r_sum[r], pe.r_est[r]};
    ncand += pe.r_ncand[r];
    if (pre_better(kk, best)) best = kk;
  }
  sk[lane] = best;
  sc[lane] = ncand;
  __syncthreads();
  for (uint32_t off = 32; off > 0; off >>= 1) {
    if (lane < off) {
      if (pre_better(sk[lane + off], sk[lane])) sk[lane] = sk[lane + off];
      sc[lane] += sc[lane + off];
    }
    __syncthreads();
  }
  best = sk[0];
  ncand = sc[0];
  const uint32_t orig = pe.sorig[slot];
  const bool none = best.node < 0;
  if (lane == 0) {
    pe.o_node[orig] = best.node;
    pe.o_ncand[orig] = ncand;
    pe.o_nv[orig] = none ? 0u : best.nv;
    pe.o_npv[orig] = none ? 0u : best.npv;
    pe.o_top[orig] = none ? 0 : best.top;
    pe.o_sum[orig] = none ? 0 : best.sum;
    pe.o_est[orig] = none ? 0 : best.est;
  }
  if (none || best.nv == 0 || pe.cap == 0) return;
  // the victim list: the reprieve of step 5 on the chosen node once more
  const uint32_t k = (uint32_t)best.node, pi = pe.spod[slot];
  const int32_t P = pe.sprio[slot];
  int64_t rq[L], al[L], cur[L];
  uint32_t rpq, apres;
  pre_pod<S>(pd, pi, rq, rpq);
  pre_node<S>(nd, k, al, cur, apres);
  const uint32_t b1 = pe.boff[k + 1];
  const uint32_t js = pre_below(pe.bprio, pe.boff[k], b1, P);   // [js, b1) = exactly the potential victims
  int64_t part[L];
#pragma unroll
  for (int l = 0; l < L; ++l) part[l] = 0;
  pre_nominees_part<S>(pe.nm, k, P, lane, part);               // rule N
  for (uint32_t j = js + lane; j < b1; j += 64u) {
#pragma unroll
    for (int l = 0; l < L; ++l) part[l] = wadd(part[l], pe.breq[(size_t)l * pe.bstride + j]);
  }
#pragma unroll
  for (int l = 0; l < L; ++l) {
    int64_t v = part[l];
    for (int off = 32; off > 0; off >>= 1) v = wadd(v, (int64_t)__shfl_xor((long long)v, off, 64));
    cur[l] = wsub(cur[l], v);
  }
  uint32_t nv = 0;
  uint32_t* vout = pe.o_victims + (size_t)orig * pe.cap;
  // two passes over the same windows where the node holds violating pods (the violating entries first): the list is in reprieve order
  const bool pdb = pe.bnviol[k] != 0;
  const uint32_t npass = pdb ? 2u : 1u;
  for (uint32_t pass = 0; pass < npass; ++pass) {
    for (uint32_t base = js; base < b1; base += 64u) {
      const uint32_t j = base + lane;
      const bool have = j < b1 && (!pdb || (pe.bpdb[j] != 0) == (pass == 0));
      uint64_t live = __ballot(have);
      if (!live) continue;
      int64_t mine[L];
#pragma unroll
      for (int l = 0; l < L; ++l) mine[l] = have ? pe.breq[(size_t)l * pe.bstride + j] : 0;
      const uint32_t myid = have ? pe.bid[j] : 0u;
      while (live) {
        const uint32_t i = (uint32_t)__builtin_ctzll(live);
        live &= live - 1;
        int64_t t[L];
#pragma unroll
        for (int l = 0; l < L; ++l) t[l] = wadd(cur[l], pre_readlane64(mine[l], i));
        if (pre_holds<S>(t, al, apres, rq, rpq)) {
#pragma unroll
          for (int l = 0; l < L; ++l) cur[l] = t[l];
        } else {
          const uint32_t vid = (uint32_t)__builtin_amdgcn_readlane((int)myid, (int)i);
          if (lane == 0 && nv < pe.cap) vout[nv] = vid;
          ++nv;
        }
      }
    }
  }
}

}  // namespace bs
