// bs_preempt_commit_gang.hpp — bs_preempt_commit_gang's resolve (include/bsched.h): k_pc_resolve's walk over the slots
// (bs_preempt_commit.hpp) with the quorum of each gang's run of slots decided on the device.  A run is a maximal sequence of consecutive
// slots of one group that has a requirement (the host makes the per-slot arrays: bs_preempt_gang_runs.hpp).  After a run's last slot the
// workgroup counts the slots that got a node; if they are fewer than the run's need, the run's evictions and nominations are taken back
// out of the working state before the next slot starts (pc_gang_rollback), and the run's slots report no node.
//
// k_gang_resolve<S> restates k_pc_resolve<S>'s body line for line and calls the same pc_eval, pre_reprieve, pick and victim-walk code;
// the lines it adds are marked "gang:".  It is a kernel of its own, not a flag on k_pc_resolve: bs_preempt_commit's kernels have to
// stay the instructions they were (profiles/preempt_gang_isa_diff.txt), and a body shared between the two through an inlined template
// changed k_pc_resolve's register allocation in every instantiation.  A change to the walk goes into both.
// k_pc_scan, k_pc_nodes, k_pc_boff and k_pc_compact serve both calls as they are.
// (The name has no k_pc_ prefix on purpose: tests/test_gpu_preempt_commit.py counts the k_pc_ kernels, five per scalar-lane count.)
#pragma once
#include "bs_preempt_commit.hpp"

namespace bs {

// bs_preempt_commit_gang: what k_gang_resolve takes beside CommitDev (a kernel argument of its own: CommitDev keeps its layout)
struct GangDev {
  // per slot, made on the host with the slot arrays
  const uint32_t* s_need;   // [q] the need of the run the slot belongs to, 0 = the slot is in no run
  const uint32_t* s_rlen;   // [q] the run's length where the slot ends a run, 0 elsewhere
  // working state beside CommitDev's (tag zeroed before the resolve; slog is written before it is read)
  uint32_t* tag;            // [bstride] slot + 1 of the slot that killed the entry (dead[] keeps its type: k_pc_compact reads it)
  uint32_t* slog;           // [q][3] per slot: chosen node + 1 (0: none), and the node's vbits / nbits words as the slot found them
  // results
  uint32_t* o_placed;       // [q] by slot: placed of the run the slot ends, before the decision (zeroed)
  uint8_t* o_voided;        // [q] caller's order: the slot had a node and lost it to its run's quorum (zeroed)
};

// A run of slots [s - rlen + 1, s] missed its quorum: take it back out of the working state, so that the next slot sees a state in
// which the run never ran.  Called by every thread after the last slot's closing barrier; the caller's barrier follows.
//   - Nothing here reads o_victims (truncated at victim_cap): the run's victims are the entries whose tag names one of its slots.
//   - dv / dn are wrapping int64 sums: subtracting what a slot added (its victims' requests, recomputed from the tagged entries; its own
//     request as the commit added it) inverts the commit exactly.  vbits / nbits are ORs: each slot logged the two words it found, and
//     the slots are undone LAST FIRST, so two slots of the run on one node end at the words from before the run.
//   - Slots are dealt to waves by node (node % waves): every slot of one node is undone by one wave, in program order, with plain
//     loads and stores (no read-modify-write of one word by two waves).  Lanes go over the node's bound list.
//   - The run's nodes STAY on the dirty list.  A dirty node with zero deltas and no dead entries evaluates (pc_eval) to its base
//     answer: its working candidacy equals its base candidacy, so the n_candidates correction adds and subtracts the same 1, and its
//     key is the key the scan recorded.  k_pc_nodes writes its base request vector back, k_pc_compact keeps all its entries.
// Everything written inside this launch (slog, tag, dead, the deltas) is read with pc_ld* vector loads.
template <int S>
__device__ __forceinline__ void pc_gang_rollback(const NodesDev& nd, const PodsDev& pd, const CommitDev& pe, const GangDev& gd, uint32_t s,
                                                 uint32_t rlen, uint32_t* s_nvall) {
  constexpr int L = 4 + S;
  constexpr int kWaves = pc_threads<S>() / 64;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t N = nd.n;
  for (uint32_t i = 0; i < rlen; ++i) {
    const uint32_t r = s - i;                                        // last slot first
    const uint32_t k1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc_ld32(gd.slog + (size_t)r * 3));
    if (k1 == 0 || (k1 - 1u) % (uint32_t)kWaves != wave) continue;   // no node, or another wave's node
    const uint32_t k = k1 - 1u;
    const uint32_t orig = pe.sorig[r];
    // the slot's victims: the entries of the node that carry its tag
    int64_t part[L];
#pragma unroll
    for (int l = 0; l < L; ++l) part[l] = 0;
    uint32_t cnt = 0;
    const uint32_t b0 = pe.boff[k], b1 = pe.boff[k + 1];
    for (uint32_t base = b0; base < b1; base += 64u) {
      const uint32_t j = base + lane;
      const bool mine = j < b1 && pc_ld32(gd.tag + j) == r + 1u;
      if (mine) {
#pragma unroll
        for (int l = 0; l < L; ++l) part[l] = wadd(part[l], pe.breq[(size_t)l * pe.bstride + j]);
        pe.dead[j] = 0;
        gd.tag[j] = 0;
      }
      cnt += (uint32_t)__builtin_popcountll(__ballot(mine));
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      int64_t v = part[l];
      for (int off = 32; off > 0; off >>= 1) v = wadd(v, (int64_t)__shfl_xor((long long)v, off, 64));
      part[l] = v;
    }
    // what the commit added for the preemptor itself
    int64_t rq[L];
    uint32_t rpq;
    pre_pod<S>(pd, pe.spod[r], rq, rpq);
    if (lane < (uint32_t)L) {
      int64_t add = 0, rem = 0;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        if ((int)lane == l) {
          rem = part[l];
          add = l < 3 ? rq[l] : (l == 3 ? 1 : (((rpq >> (l - 4)) & 1u) ? rq[l] : 0));
        }
      }
      pe.dv[(size_t)lane * N + k] = wsub(pc_ld64(pe.dv + (size_t)lane * N + k), rem);
      pe.dn[(size_t)lane * N + k] = wsub(pc_ld64(pe.dn + (size_t)lane * N + k), add);
    }
    if (lane == 0) {
      pe.vbits[k] = pc_ld32(gd.slog + (size_t)r * 3 + 1);
      pe.nbits[k] = pc_ld32(gd.slog + (size_t)r * 3 + 2);
      atomicSub(s_nvall, cnt);
      // the slot's answer: no node (n_candidates keeps what the slot saw; the host zeroes the victim row of a slot without victims)
      pe.o_node[orig] = -1;
      pe.o_nv[orig] = 0;
      pe.o_npv[orig] = 0;
      pe.o_top[orig] = 0;
      pe.o_sum[orig] = 0;
      pe.o_est[orig] = 0;
      gd.o_voided[orig] = 1;
    }
  }
}

// k_pc_resolve<S>'s walk (stages A-D, three barriers a slot: see bs_preempt_commit.hpp) with the gang bookkeeping: wave 0 tags the entries
// it kills, logs the chosen node and the two bit words it found, and counts the run's placed slots in LDS; at a run's last slot every
// thread reads the count after the slot's closing barrier, a missed run is rolled back, and one more barrier closes the run.
template <int S>
__global__ __launch_bounds__(pc_threads<S>()) void k_gang_resolve(NodesDev nd, PodsDev pd, CommitDev pe, GangDev gd) {
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
        }
      }
      if (lane == 0) s_nres = 0;
    }
    __syncthreads();
    // gang: the run's quorum, after its last slot: one more barrier at run ends only (rlen is the same for every thread)
    const uint32_t rlen = gd.s_rlen[s];
    if (rlen) {
      const uint32_t placed = s_placed;
      if (placed < gd.s_need[s]) pc_gang_rollback<S>(nd, pd, pe, gd, s, rlen, &s_nvall);
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
