// bs_preempt_clear.hpp — BS_PREEMPT_CLEAR_LOWER's resolve (include/bsched.h, rule C): when a slot stands on a node, the rows of the
// nominated-pod table on that node with a priority below the slot's are cleared, and no later slot of the call counts them (upstream's
// getLowerPriorityNominatedPods after pickOneNodeForPreemption).  The kernel uses the rule's threshold form: T[k] is the priority of the
// first standing slot on node k in slot order (priority-descending: the highest of all takers), INT32_MIN while nobody stands there, and
// slot s on node k adds the rows with priority >= max(P_s, T[k]).
//
// k_nc_resolve<S> restates k_gang_resolve<S>'s walk (bs_preempt_commit_gang.hpp) line for line; the lines it adds are marked "clear:".
// It is a kernel of its own for the reason k_gang_resolve is one (that header, lines 7-12): the existing kernels stay the instructions
// they are, and pc_eval gets a sibling here (pc_eval_nc) instead of a parameter.  It serves BOTH calls: bs_preempt_commit hands it
// all-zero s_need / s_rlen, with which no slot is in a run and the gang lines do nothing.  The host launches it only when the flag is
// set and the table has rows (nom_view(c) non-null); otherwise today's kernels run.  A change to the walk goes into all three.
//
// Only two places read the threshold: the re-evaluation of a DIRTY node, and stage D's nominee sum on the winning node.  Clean nodes have
// T = INT32_MIN, so max(P, T) = P and their evaluation is rule N's.  The clean-chunk argument of the records is untouched for the same
// reason: the threshold of a node changes only when some slot takes the node, which puts the node on the dirty list, and the records are
// only trusted for nodes that are not on it.  (After a voided run a node stays dirty with T restored: it is re-evaluated with the T it
// had before the run, which is the base answer when that is INT32_MIN.)
//
// Working state beside CommitDev's and GangDev's (ClearDev; both keep their layouts).  thr is stored biased (priority ^ 0x80000000, an
// unsigned order), so the zeroed working-state block means INT32_MIN.  Wave 0 writes thr and first at the commit stage, after the slot's
// second barrier; everyone reads them after the slot's closing barrier with pc_ld32 vector loads, never through the scalar cache.
// The rollback of a voided run restores the two words last slot first from the slot log, by the wave that restores vbits / nbits.
#pragma once
#include "bs_preempt_commit_gang.hpp"

namespace bs {

struct ClearDev {
  // working state (zeroed before the resolve)
  uint32_t* thr;            // [n] T[k] ^ 0x80000000: 0 = INT32_MIN = nobody stands on the node
  uint32_t* first;          // [n] slot + 1 of the first standing slot on the node, 0 = none
  uint32_t* clog;           // [q][2] per slot that got a node: the node's thr / first words as the slot found them (beside gd.slog)
};

__device__ __forceinline__ uint32_t nc_bias(int32_t p) { return (uint32_t)p ^ 0x80000000u; }
// the nominee priority of a slot of priority P on a node whose threshold word is tw: max(P, T)
__device__ __forceinline__ int32_t nc_nominee_prio(int32_t P, uint32_t tw) { return (int32_t)(max(nc_bias(P), tw) ^ 0x80000000u); }

// pc_eval (bs_preempt_commit.hpp) with the working-state evaluation's nominee priority as an argument: Pn = max(P, T[k]) on a dirty node,
// Pn = P on a clean one.  The base-state answer of a dirty node is what the scan counted: the rows at P.
template <int S>
__device__ bool pc_eval_nc(const NodesDev& nd, const CommitDev& pe, uint32_t k, int32_t P, int32_t Pn, const int64_t (&rq)[4 + S], uint32_t rpq,
                           uint32_t cls, int32_t qg, bool dirty, PreKey& key, int32_t& dcand) {
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
  pre_nominees<S>(pe.nm, k, Pn, cur);                           // clear: rule C on top of rule N (local: dv / dn never hold the rows)
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

// clear: after pc_gang_rollback took the run [s - rlen + 1, s] out of the working state: the thresholds and first-taker words of its
// nodes go back to what each slot found, last slot first, by the wave pc_gang_rollback dealt the node to (node % waves: every slot of
// one node is undone by one wave in program order, plain stores).  A row that a standing slot before the run had cleared stays cleared:
// that slot's threshold is what the run's first slot logged.
template <int S>
__device__ __forceinline__ void nc_rollback(const GangDev& gd, const ClearDev& cd, uint32_t s, uint32_t rlen) {
  constexpr int kWaves = pc_threads<S>() / 64;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t i = 0; i < rlen; ++i) {
    const uint32_t r = s - i;
    const uint32_t k1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc_ld32(gd.slog + (size_t)r * 3));
    if (k1 == 0 || (k1 - 1u) % (uint32_t)kWaves != wave) continue;
    if (lane == 0) {
      cd.thr[k1 - 1u] = pc_ld32(cd.clog + (size_t)r * 2);
      cd.first[k1 - 1u] = pc_ld32(cd.clog + (size_t)r * 2 + 1);
    }
  }
}

template <int S>
__global__ __launch_bounds__(pc_threads<S>()) void k_nc_resolve(NodesDev nd, PodsDev pd, CommitDev pe, GangDev gd, ClearDev cd) {
  constexpr int L = 4 + S;
  constexpr int kPcThreads = pc_threads<S>();
  constexpr int kWaves = kPcThreads / 64;
  __shared__ uint32_t s_res[kPcThreads];        // chunks to rescan this slot (at most nchunks; capped below by the walk)
  __shared__ uint32_t s_nres, s_ndirty, s_nvall;
  __shared__ uint32_t s_placed;                 // gang: slots of the current run that got a node
  __shared__ PreKey s_key[kWaves];
  __shared__ int32_t s_dc[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t N = nd.n;
  if (t == 0) { s_nres = 0; s_ndirty = 0; s_nvall = 0; s_placed = 0; }
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
      int32_t Pn = P;                              // clear: the nominee priority, max(P, T[k]) on a dirty node
      if (i < nd_) {
        k = pc_ld32(pe.dlist + i);
        dirty = true;
        Pn = nc_nominee_prio(P, pc_ld32(cd.thr + k));
      } else {
        const uint32_t x = i - nd_, c = s_res[x / pe.chunk_nodes];
        k = c * pe.chunk_nodes + x % pe.chunk_nodes;
        if (k >= N || pc_ld8(pe.dirty + k)) continue;
        dirty = false;
      }
      PreKey kk;
      if (pc_eval_nc<S>(nd, pe, k, P, Pn, rq, rpq, cls, qg, dirty, kk, dc) && pre_better(kk, best)) best = kk;
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
          if (pc_eval_nc<S>(nd, pe, k, P, P, rq, rpq, cls, qg, false, kk, dc) && pre_better(kk, best)) best = kk;
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
        if (none) gd.slog[(size_t)s * 3] = 0;                      // gang: the log's node word; the run's placed count
        else if (gd.s_need[s]) s_placed = s_placed + 1;
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
        // clear: the two words as this slot finds them (vector loads; every lane loads the same word: kept in scalar registers)
        const uint32_t mthr = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc_ld32(cd.thr + k));
        const uint32_t mfirst = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc_ld32(cd.first + k));
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
        pre_nominees_part<S>(pe.nm, k, nc_nominee_prio(P, mthr), lane, part);   // clear: rule C on top of rule N: max(P, T[k])
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
            if ((vmask >> lane) & 1ull) {
              pe.dead[j] = 1;
              gd.tag[j] = s + 1u;                                  // gang: the entry's owner
            }
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
          gd.slog[(size_t)s * 3] = k + 1u;                         // gang: the node and the two words as this slot found them
          gd.slog[(size_t)s * 3 + 1] = mvb;
          gd.slog[(size_t)s * 3 + 2] = mnb;
          cd.clog[(size_t)s * 2] = mthr;                           // clear: ... and the threshold and first-taker words
          cd.clog[(size_t)s * 2 + 1] = mfirst;
          if (nc_bias(P) > mthr) cd.thr[k] = nc_bias(P);           // clear: the slot stands: T[k] rises (only ever from nobody)
          if (mfirst == 0) cd.first[k] = s + 1u;
        }
      }
      if (lane == 0) s_nres = 0;
    }
    __syncthreads();
    // gang: the run's quorum, after its last slot: one more barrier at run ends only (rlen is the same for every thread)
    const uint32_t rlen = gd.s_rlen[s];
    if (rlen) {
      const uint32_t placed = s_placed;
      if (placed < gd.s_need[s]) {
        pc_gang_rollback<S>(nd, pd, pe, gd, s, rlen, &s_nvall);
        nc_rollback<S>(gd, cd, s, rlen);                           // clear: the run's clearings are taken back with it
      }
      __syncthreads();
      if (t == 0) {
        gd.o_placed[s] = placed;
        s_placed = 0;
      }
    }
  }
  if (t == 0) { pe.info[0] = s_ndirty; pe.info[1] = s_nvall; }
}

}  // namespace bs
