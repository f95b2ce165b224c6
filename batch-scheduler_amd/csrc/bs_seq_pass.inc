// bs_seq_pass.inc — the body of k_seq_pass (bs_seq.hpp), included once by each of its four kernel templates: k_seq_pass<TS> (bs_seq_run) with
// `constexpr bool NOM = false`, k_seq_pass<TS, true> (bs_seq_run_nominated, rule S) with NOM = true and the kernel argument `nom`,
// k_seq_scored<TS> (bs_seq_run_scored, rule P) with SCORE = true and the kernel argument `sco`, k_seq_sp<TS>
// (bs_seq_run_scored_nominated, rule SP) with both flags and both arguments; and by the two sampled templates k_seq_sampled<TS> and
// k_seq_sampled_nom<TS> (rule F over rule P and over rule SP) with SCORE and SAMPLE = true and the kernel argument `smp`; every
// sampled-only line sits behind `if constexpr (SAMPLE)`.  Every NOM-only line sits behind
// `if constexpr (NOM)`, every scored-only line behind `if constexpr (SCORE)`; what the scored pass must not touch (the first-fit cursors,
// `mono`) behind `if constexpr (!SCORE)`.  A shared __device__ function would be the usual form; the flag-less kernels then come
// out as other instructions than before (inlining a by-reference body is not the same input to the optimiser), and bs_seq_run's kernels
// are required to stay instruction-identical.  Kernel parameters in scope: pods, gr, nd, sq, prm.
  // The scored kernels for more than kSeqScoredFullLanes scalar lanes are built lean (no scratch memory): no table summaries in LDS (every
  // PreFilter scan walks the list in rounds, as with prm.cache_slots == 0) and no wave-uniform copy of the pod's scalar request lanes (seq_pick_scored).
  constexpr bool kLeanScored = SCORE && TS > kSeqScoredFullLanes;
  extern __shared__ unsigned long long s_keys[];             // [G] when prm.keys_in_lds
  __shared__ SeqShared sh_;
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), S = sh.S();
  const uint32_t P = pods.p, G = gr.g, N = nd.n;
  const uint32_t gate = prm.eph_gate;
  const bool t0 = threadIdx.x == 0;

  // ---- prologue: keys, left arrays, meta words, first-fit bounds, per-gang bookkeeping
  for (uint32_t g = threadIdx.x; g < G; g += kSeqBlock) {
    const unsigned long long k = seq_key(g, gr.flags[g], gr.min_member[g], gr.status_scheduled[g], gr.matched[g]);
    if (prm.keys_in_lds) s_keys[g] = k; else sq.keys[g] = k;
    sq.head[g] = 0;
    sq.nwait[g] = 0;
    sq.slot_of[g] = BS_INF;
    sq.t_first[g] = ~0ull;
  }
  for (uint32_t i = threadIdx.x; i < P; i += kSeqBlock) { sq.pod_node[i] = -1; if (prm.filter_deny) sq.last_permitted[i] = 0; }
  if (t0) { sh_.hit_w[0] = BS_INF; sh_.hit_w[1] = BS_INF; }
  if (threadIdx.x < kSeqPruneTiles / 32) sh_.tight[threadIdx.x] = 0;
  SeqNomShared* ns = nullptr;
  if constexpr (NOM) {
    ns = reinterpret_cast<SeqNomShared*>(reinterpret_cast<unsigned char*>(s_keys) + nom.lds_off);
    if (threadIdx.x < kSeqPruneTiles / 32) ns->wild[threadIdx.x] = 0;
    if constexpr (!SCORE) {                                  // (grow and cur_prio[] serve the first-fit cursors alone)
    if (t0) ns->grow = 0u;
    for (uint32_t e = threadIdx.x; e < kSeqCursors; e += kSeqBlock) ns->cur_prio[e] = 0;
    }
    __syncthreads();                                         // (wild[] is or-ed into by the loop below)
  }
  for (uint32_t base = 0; base < N; base += kSeqBlock) {
    const uint32_t n = base + threadIdx.x;
    const bool valid = n < N;
    const uint32_t nn = valid ? n : N - 1u;
    const uint32_t fl = nd.flags[nn], ap = nd.apres[nn], rp = sq.rpres[nn];
    long long f0 = INT64_MIN, f1 = INT64_MIN;
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
      if (j < L) {
        const int64_t a = nd.alloc[(size_t)j * nd.stride + nn], q = sq.nreq[(size_t)j * nd.stride + nn];
        if (valid) {
          sq.left07[(size_t)j * nd.stride + n] = wsub(scale_f32(a, 0.7f), q);
          sq.left10[(size_t)j * nd.stride + n] = wsub(scale_f32(a, 1.0f), q);
        }
        if (valid && fl == 0u) {
          if (j == 0) f0 = wsub(a, q);
          if (j == 1) f1 = wsub(a, q);
        }
      }
    }
    if (valid) sq.nmeta[n] = ((fl & BS_NODE_SKIP_MASK) ? 0u : 1u) | ((fl & BS_NODE_TAINT_ERR) ? 2u : 0u) | ((ap & rp) << 4);
    if (prm.prune) {
      const long long m0 = readlane63_i64(wave_max_i64_lane63(f0)), m1 = readlane63_i64(wave_max_i64_lane63(f1));
      const long long m2 = readlane63_i64(wave_max_i64_lane63(f0 == INT64_MIN ? INT64_MIN : seq_joint(f0, f1)));
      if (lane_id() == 0 && n < N) { sh_.pmax[0][n >> 6] = m0; sh_.pmax[1][n >> 6] = m1; sh_.pmax[2][n >> 6] = m2; }
      if constexpr (NOM) {
        // The bounds are upper bounds of the RAW free cpu / memory; the fit test sees raw - (row sum).  That is below raw, for every
        // priority and every set of consumed rows, as long as every row on the node asks for 0 <= cpu, memory < 2^40 (at most 2^16 rows: the
        // sum stays below 2^56) and the raw free values are above -2^62 (no wrap; they only fall by requests that fitted).  A tile with a
        // node where that does not hold is never pruned and never tightened.
        bool wild = false;
        if (valid && fl == 0u && nom.view) {
          const NomView nm = *nom.view;
          for (uint32_t r = nm.nhead[n]; r != kNmNone; r = nm.nnext[r]) {
            const int64_t v0 = nm.nreq[r], v1 = nm.nreq[(size_t)nm.nstride + r];
            wild = wild || v0 < 0 || v0 >= (1ll << 40) || v1 < 0 || v1 >= (1ll << 40) || f0 < -(1ll << 62) || f1 < -(1ll << 62);
          }
        }
        if (__ballot(wild) != 0ull && lane_id() == 0 && n < N) {
          sh_.pmax[0][n >> 6] = INT64_MAX; sh_.pmax[1][n >> 6] = INT64_MAX; sh_.pmax[2][n >> 6] = INT64_MAX;
          atomicOr(&ns->wild[n >> 11], 1u << ((n >> 6) & 31u));
        }
      }
    }
  }
  if constexpr (NOM && !SCORE) {
    // The first-fit cursors rest on "the room a pod sees only shrinks": with every assume step, and from a pod of priority Pc to one of
    // P <= Pc, who sees every row that pod saw and more.  A row takes room only if its lanes are not negative and no sum wraps.  That holds
    // when every row asks for 0 <= v < 2^40 on EVERY lane (at most 2^16 rows: a sum stays below 2^56) and, on every schedulable node that
    // holds rows, every lane's free value is above -2^62 (allocatable too where the requests lack a scalar key) and the pods lane's request
    // below 2^62; afterwards free values only fall by requests that fitted.  Otherwise a row may GROW the room (a negative lane, two rows of
    // 2^63 - 1): the pass then runs without cursors, as it does once a pod's negative request has freed capacity.
    bool grow = false;
    if (nom.view) {
      const NomView nm = *nom.view;
      constexpr long long kBig = 1ll << 62;
      for (uint32_t r = threadIdx.x; r < nom.rows; r += kSeqBlock) {
#pragma unroll
        for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
          if (j < L) {
            const int64_t v = nm.nreq[(size_t)j * nm.nstride + r];
            grow = grow || v < 0 || v >= (1ll << 40);
          }
        }
      }
      for (uint32_t n = threadIdx.x; n < N; n += kSeqBlock) {
        if (nd.flags[n] != 0u || nm.nhead[n] == kNmNone) continue;
        const uint32_t rp = sq.rpres[n];
#pragma unroll
        for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
          if (j < L) {
            const int64_t a = nd.alloc[(size_t)j * nd.stride + n], q = sq.nreq[(size_t)j * nd.stride + n];
            grow = grow || wsub(a, q) < -kBig || (j >= 4 && !((rp >> (j - 4)) & 1u) && a < -kBig);   // (a scalar key the requests lack counts as 0)
            if (j == 3) grow = grow || q > kBig || q < -kBig;
          }
        }
      }
    }
    if (grow) atomicOr(&ns->grow, 1u);
  }
  // table summaries (see seq_scan_cached): which table sits in which slot, how many of its tiles wait for a refresh
  const uint32_t ntiles = (N + 63u) >> 6;
  const SeqCache ch = seq_cache_view(reinterpret_cast<unsigned char*>(s_keys) + prm.cache_off, ntiles, prm.cache_slots, sh);
  uint32_t slot_key[kSeqCacheSlots], slot_age[kSeqCacheSlots], age_ctr = 0;
#pragma unroll
  for (uint32_t c = 0; c < kSeqCacheSlots; ++c) { slot_key[c] = BS_INF; slot_age[c] = 0; }
  if constexpr (!SCORE)
  for (uint32_t e = threadIdx.x; e < kSeqCursors; e += kSeqBlock) { sh_.cur_kn[e] = 0ull; sh_.cur_fc[e] = 0u; }   // (ordered by the barrier in front of the loop)
  uint32_t smp_cur = 0;                                      // rule F: the cursor of the next walk, wave-uniform and the same in every wave
  if constexpr (SAMPLE) smp_cur = smp.s0;
  uint32_t hit_par = 0;                                      // which of the two early-stop words the next search uses
  bool mono = true;                                          // no assumed request has freed capacity so far: the first-fit cursors hold
  bool stores_pending = true;                                // an assume step (or the prologue) stored node state nobody has waited for yet
  int32_t sop_leader = prm.sop_leader0;                      // sop.maxFinishedPG / maxPGStatus (core.go:58-59), stale between calls
  uint32_t n_released = 0;
  unsigned long long n_pick = 0, n_scan = 0, n_rounds = 0, n_tiles = 0, n_folds = 0, n_builds = 0;
  // findMaxPG's answer is kept until a key changes (capture, Permit, release)
  // ... and a change of ONE key only matters when it beats the winner's (fold_top = the winner's key, 0 = repeat the fold on any change)
  bool fold_valid = false, fold_panic = false;
  int32_t fold_leader = -1;
  unsigned long long fold_top = 0;
  // register-resident group state: the pod's own group (own_of) and the leader's (ldr_of); -1 = nothing cached
  SeqGroup own, ldr;
  seq_group_zero(own, sh);
  seq_group_zero(ldr, sh);
  int32_t own_of = -1, ldr_of = -1;
  uint32_t wl_cnt = 0;                                       // waiting pods of group own_of recorded in the LDS list
  bool wl_ok = true;                                         // ... and the list holds ALL of them (nothing waited before the group became current)
  const unsigned long long clk0 = (unsigned long long)wall_clock64();
  BS_SEQ_FULL_BARRIER();
  if constexpr (NOM && !SCORE) mono = uni32(ns->grow) == 0u;           // (see the prologue: a row that may grow the room switches the cursors off)
#ifdef BS_SEQ_PROBE
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl = (unsigned long long)__builtin_readcyclecounter();
  if (t0) { for (int k = 0; k < 32; ++k) sh_.ph2[k] = 0; sh_.tl2 = tl; }
#endif

  for (uint32_t i = 0; i < P; ++i) {
    const uint32_t pw = i % kSeqPodWin;
    if (pw == 0u) {                                          // the next window of pod fields (every wave is through with the last one)
      if (i) lds_barrier();
      seq_stage_pods(pods, gr, sq, sh_, i, sh);
      if constexpr (NOM) {                                   // two more immutable per-pod fields
        if (threadIdx.x < kSeqPodWin) {
          const uint32_t p = min(i + threadIdx.x, P - 1u);
          ns->pw_prio[threadIdx.x] = nom.pprio[p];
          ns->pw_own[threadIdx.x] = nom.pown[p];
        }
      }
    }
    lds_barrier();                                           // keys / bounds / wait list as the previous pod left them
    BS_SEQ_T(6);
    BS_SEQ_P(0);
    const int32_t gi = (int32_t)uni32((uint32_t)sh_.pw_group[pw]);
    const uint32_t pflags = uni32(sh_.pw_flags[pw]);
    const uint32_t pod_mm = uni32(sh_.pw_mm[pw]);            // MinMember of the pod's group (0 if it has none)
    const bool grouped = gi >= 0 && (uint32_t)gi < G;
    uint32_t code;
    uint32_t fk = BS_K_NOT_SCANNED;
    bool scan = false, pct07 = false, deny = false;
    uint32_t tcls = 0;
    Res R;
    res_zero(R, sh);
    // READ PHASE.  A group that is not in registers costs one round trip (behind a full barrier: thread 0's stores of
    // earlier pods have landed); the leader the previous call left behind is fetched in the same trip.
    {
      const bool miss_own = grouped && gi != own_of;
      const bool miss_ldr = sop_leader >= 0 && sop_leader != gi && sop_leader != ldr_of;
      if (miss_own || miss_ldr) {
        BS_SEQ_FULL_BARRIER();
        if (miss_own) {
          if (gi == ldr_of) { const uint32_t h = seq_raw32(&sq.head[gi]), nw = seq_raw32(&sq.nwait[gi]); const uint64_t tf = seq_raw64(&sq.t_first[gi]);
                              own = ldr; own.head = uni32(h); own.nwait = uni32(nw); own.seen = uni64(tf) != ~0ull; }
          else seq_group_load(sq, gr, G, (uint32_t)gi, sh, own);
          own_of = gi;
          wl_cnt = 0;
          wl_ok = (own.nwait & ~kSeqHasRecord) == 0;
        }
        if (miss_ldr) { seq_group_load(sq, gr, G, (uint32_t)sop_leader, sh, ldr); ldr_of = sop_leader; }
      }
    }
    if (grouped && !own.seen) {
      if (t0) sq.t_first[gi] = (unsigned long long)wall_clock64() - clk0;
      own.seen = true;
    }
    BS_SEQ_T(0);
    BS_SEQ_P(1);
    uint32_t gflags = grouped ? own.flags : 0u;              // of the pod's own group, as this PreFilter call leaves them
    const uint32_t gmatched = grouped ? own.matched : 0u, gsc = grouped ? own.sc : 0u;

    if (gi == BS_POD_NOT_GROUPED) code = BS_PF_PASS_NOT_GROUPED;                                    // core.go:89-92
    else if (pflags & BS_POD_LAST_PERMITTED) code = BS_PF_PASS_LAST_PERMITTED;                      // :95-98
    else if (!grouped) code = BS_PF_ERR_PG_NOT_FOUND;                                               // :100-103
    else if (gflags & BS_GROUP_DENIED) code = BS_PF_ERR_DENIED;                                     // :105-110
    else {
      // fillOccupiedObj, core.go:477-512
      const uint32_t mm = pod_mm;
      uint32_t nf = gflags;
      if (!(gflags & BS_GROUP_HAS_POD)) { nf |= BS_GROUP_HAS_POD; own.cls = uni32(sh_.pw_cls[pw]); }           // :486-488
      if (!(gflags & BS_GROUP_HAS_MINRES)) { nf |= BS_GROUP_HAS_MINRES; seq_pod_require(sh_, pw, sh, gate, own.mr); }   // :489-493
      const uint64_t occ = own.occ, refs = uni64(sh_.pw_owner[pw]);
      const bool take_owner = occ == 0 && refs != 0;                                                 // :494-501
      const bool occupied = occ != 0 && (refs == 0 || refs != occ);                                  // :503-510
      if (nf != gflags || take_owner) {
        if (t0) {                                            // (nobody reads these words from memory while the group is current)
          if (!(gflags & BS_GROUP_HAS_POD)) sq.g_cls[gi] = own.cls;
          if (!(gflags & BS_GROUP_HAS_MINRES)) {
#pragma unroll
            for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
              if (j < L) sq.g_minres[(size_t)j * G + gi] = own.mr.v[j];
            sq.g_mrpres[gi] = own.mr.present;
          }
          if (take_owner) sq.g_occ[gi] = refs;
          if (nf != gflags) sq.g_flags[gi] = (uint8_t)nf;
        }
        if (take_owner) own.occ = refs;
        if (nf != gflags) {
          const unsigned long long k = seq_key((uint32_t)gi, nf, mm, gsc, gmatched);
          if (t0) { if (prm.keys_in_lds) s_keys[gi] = k; else sq.keys[gi] = k; }
          if (fold_top == 0ull || k > fold_top) fold_valid = false;   // the capture is a candidate of this very findMaxPG: it only matters if it wins
          gflags = nf;
          own.flags = nf;
          if (prm.keys_in_lds) lds_barrier(); else BS_SEQ_FULL_BARRIER();
        }
      }
      BS_SEQ_T(1);
      if (occupied) code = BS_PF_ERR_OCCUPIED;                                                       // :113-115
      else {
        if (!fold_valid) {
          seq_find_max(gr, sq, prm, sh_, s_keys, fold_leader, fold_panic, fold_top);                 // :118-123
          fold_valid = true;
          n_folds++;
        }
        BS_SEQ_T(2);
        const int32_t leader = fold_leader;
        if (fold_panic) code = BS_PF_PANIC_DIV0;
        else {
          sop_leader = leader;                                                                       // :121-122
          if (leader < 0) code = BS_PF_PASS_NO_MAX;                                                  // :127-130
          else {
            if (leader != gi && leader != ldr_of) {          // (the leader changed: one more round trip)
              BS_SEQ_FULL_BARRIER();
              seq_group_load(sq, gr, G, (uint32_t)leader, sh, ldr);
              ldr_of = leader;
            }
            const uint32_t lmatched = leader == gi ? gmatched : ldr.matched;                         // :132-135
            if (lmatched == 0) {                                                                     // :136-147
              // getPreAllocatedResource(pgs, 0), core.go:774-793
              const int64_t nfin = (int64_t)mm - (int64_t)gsc;
              if (nfin > 0) {
                Res times;
#pragma unroll
                for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
                  if (j < L) times.v[j] = wmul(own.mr.v[j], nfin);
                times.present = own.mr.present;
                res_add(R, times, sh, gate);
              }
              if (R.v[BS_LANE_PODS] == 0) R.v[BS_LANE_PODS] = (int64_t)mm + 1;
              scan = true;
              tcls = own.cls;
              pct07 = false;
              code = BS_PF_PASS_FIRST_FITS;
            } else if (leader == gi) code = BS_PF_PASS_IS_MAX;                                       // :150-155
            else {                                                                                   // :157-166
              const uint32_t lmm = ldr.mm;
              const int64_t nfin = (int64_t)lmm - (int64_t)lmatched;                                 // matched != 0: :778-779
              if (nfin > 0 && (ldr.flags & BS_GROUP_HAS_MINRES)) {
                Res times;
#pragma unroll
                for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
                  if (j < L) times.v[j] = wmul(ldr.mr.v[j], nfin);
                times.present = ldr.mr.present;
                res_add(R, times, sh, gate);
              }
              if (R.v[BS_LANE_PODS] == 0) R.v[BS_LANE_PODS] = (int64_t)lmm + 1;
              Res cur;
              seq_pod_require(sh_, pw, sh, gate, cur);                                               // :158
              res_add(R, cur, sh, gate);                                                             // :159
              scan = true;
              tcls = ldr.cls;
              pct07 = true;
              code = BS_PF_PASS_RESERVE_FITS;
            }
          }
        }
      }
    }

    // ---- Filter's per-pod half (core.go:170-180, :524-544) with sop.maxPGStatus as this PreFilter call left it
    SeqPick q;
    q.fl = BS_FL_PASS_NOT_GROUPED;
    q.ff = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { q.FR[j] = 0; q.FM[j] = 0; }
    if (BS_PF_IS_PASS(code) && prm.run_filter) {
      if (gi == BS_POD_NOT_GROUPED) q.fl = BS_FL_PASS_NOT_GROUPED;
      else if (!grouped) q.fl = BS_FL_ERR_PG_NOT_FOUND;
      else if (sop_leader < 0) q.fl = BS_FL_PANIC_NIL_MAX;
      else if (sop_leader == gi) q.fl = BS_FL_PASS_IS_MAX;
      else {
        // (sop_leader is in ldr: fetched at the top, or by the fold branch above)
        if (!(ldr.flags & BS_GROUP_HAS_MINRES)) q.fl = BS_FL_PASS_NO_MINRES;
        else {
          Res ms, cur;
          res_zero(ms, sh);
          res_add(ms, ldr.mr, sh, gate);                                                             // :526-527
          seq_pod_require(sh_, pw, sh, gate, cur);                                                   // :551
          res_add(cur, ms, sh, gate);                                                                // :552
          q.fl = BS_FL_EVALUATED;
#pragma unroll
          for (int j = 0; j < 4; ++j) { q.FR[j] = cur.v[j]; q.FM[j] = ms.v[j]; }
#pragma unroll
          for (uint32_t s = 0; s < BS_MAX_SCALARS; ++s) {
            if (s < S) {
              if ((cur.present & (1u << s)) && cur.v[4 + s] != 0) q.ff |= 1u;
              if ((ms.present & (1u << s)) && ms.v[4 + s] != 0) q.ff |= 2u;
            }
          }
        }
      }
    }

    // ---- the node scan of this PreFilter call
    BS_SEQ_T(0);
    BS_SEQ_P(2);
    bool drained = false;                                    // this pod has already waited for the stores of earlier assume steps
    if (scan) {
      uint32_t first_k;
      if (stores_pending) { __syncthreads(); stores_pending = false; }
      BS_SEQ_P(3);
      drained = true;
      if (!kLeanScored && prm.cache_slots) {
        const uint32_t key = (tcls << 1) | (pct07 ? 1u : 0u);
        uint32_t sel = BS_INF;
#pragma unroll
        for (uint32_t c = 0; c < kSeqCacheSlots; ++c)
          if (c < prm.cache_slots && slot_key[c] == key) sel = c;
        if (sel == BS_INF) {                                 // not cached: the least recently used slot takes the table (summarised from scratch)
          uint32_t best_age = BS_INF;
#pragma unroll
          for (uint32_t c = 0; c < kSeqCacheSlots; ++c) {
            if (c < prm.cache_slots) {
              const uint32_t a = slot_key[c] == BS_INF ? 0u : slot_age[c] + 1u;
              if (a < best_age) { best_age = a; sel = c; }
            }
          }
          seq_cache_build<TS>(nd, sq, prm, sh_, ch, sel, tcls, pct07);
#pragma unroll
          for (uint32_t c = 0; c < kSeqCacheSlots; ++c)
            if (c == sel) slot_key[c] = key;
          n_builds++;
        }
        age_ctr++;
#pragma unroll
        for (uint32_t c = 0; c < kSeqCacheSlots; ++c)
          if (c == sel) slot_age[c] = age_ctr;
        BS_SEQ_P(4);
        first_k = seq_scan_cached<TS>(nd, sq, prm, sh_, ch, sel, tcls, pct07, R, hit_par, n_rounds);
      } else {
        first_k = seq_scan<TS>(nd, sq, prm, sh_, tcls, pct07, R, n_rounds);
      }
      n_scan++;
      fk = first_k == BS_INF ? BS_K_NONE : first_k;
      if (first_k == BS_INF) {                               // compareClusterResourceAndRequire false: AddToDenyCache (:142,:163)
        code = code == BS_PF_PASS_FIRST_FITS ? BS_PF_REJECT_FIRST : BS_PF_REJECT_RESERVE;
        deny = true;
      }
    }
    // ---- node choice + assume (WRITE PHASE from here on)
    BS_SEQ_T(3);
    BS_SEQ_P(8);
    uint32_t at = BS_INF;
    if (BS_PF_IS_PASS(code) && (grouped || gi == BS_POD_NOT_GROUPED)) {   // (a labelled pod of an unknown group, here on its lastPermittedPod entry:
      //                                                                   Permit answers "can not found pod group", core.go:275-278, and the framework forgets it)
      q.pcls = uni32(sh_.pw_cls[pw]);
      q.ppres = uni32(sh_.pw_pres[pw]);
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) q.preq[j] = j < L ? (int64_t)uni64((uint64_t)sh_.pw_req[j][pw]) : 0;
      if constexpr (kLeanScored) {                           // (the lean search reads the scalar lanes from the staged window itself)
#pragma unroll
        for (uint32_t j = 4; j < BS_MAX_LANES; ++j) q.preq[j] = 0;
      }
      if (prm.filter_deny && grouped) {
        // ---- Filter's TTL writes (core.go:170-191), every node of the list offered (the batch form's rule, bs_batch_run): a node whose
        // Filter fails — getLeftResource nil (:545-548) or neither case 2 nor case 3 (:562-563) — deny-lists the group (:183-185) for the
        // gang's later pods; a node whose Filter passes leaves the pod's lastPermittedPod entry (:188).  The pod itself goes on.
        bool failed = false, passed = false;
        if (q.fl == BS_FL_EVALUATED) {
          if (!drained && stores_pending) { __syncthreads(); stores_pending = false; }      // the assume steps of earlier pods have landed
          drained = true;
          for (uint32_t n = threadIdx.x; n < N; n += kSeqBlock) {
            bool c2 = !(q.ff & 1u), c3h = !(q.ff & 2u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int64_t left = wsub(nd.alloc[(size_t)j * nd.stride + n], sq.nreq[(size_t)j * nd.stride + n]);   // getLeftResource :460-463
              c2 = c2 && left >= q.FR[j];
              c3h = c3h && left >= q.FM[j];
            }
            const bool ok = !(nd.flags[n] & (BS_NODE_NIL | BS_NODE_NO_NODE)) && (c2 || !c3h);
            failed = failed || !ok;
            passed = passed || ok;
          }
          const uint32_t par = hit_par & 1u;
          const uint32_t wbits = (__ballot(failed) ? 1u : 0u) | (__ballot(passed) ? 2u : 0u);
          if (lane_id() == 0) sh_.fdw[par][wave_id()] = wbits;
          lds_barrier();
          uint32_t all = 0;
#pragma unroll
          for (int ww = 0; ww < kSeqWaves; ++ww) all |= sh_.fdw[par][ww];
          all = uni32(all);
          failed = all & 1u;
          passed = all & 2u;
        } else if (q.fl < 16u) passed = N != 0u;                                             // case 1 / no MinResources: nil on every node
        if (failed) deny = true;                                                             // (written out with PreFilter's own entries below)
        if (passed && t0) sq.last_permitted[i] = 1;
      }
      SeqAssumed as;
      if constexpr (SCORE) {
        // rule P: the candidate with the largest total, ties to the lowest index — a full search, so no cursor and no `mono`
        uint32_t sc_total = 0, sc_nfit = 0;
        if constexpr (SAMPLE) {
          // rule F: the candidates of the form underneath (rule P's, or rule S's under NOM), walked in visit order from the cursor; the first K
          // are kept and scored, the walk ends at the (K+1)-th; the cursor moves by the nodes visited.  D6's consume as in rule SP.
          SeqPickNom pn{};
          if constexpr (NOM) { pn.nom = &nom; pn.ns = ns; pn.prio = (int32_t)uni32((uint32_t)ns->pw_prio[pw]); pn.own = uni32(ns->pw_own[pw]); }
          uint32_t sm_visited = 0;
          at = seq_pick_sampled<TS, NOM>(nd, sq, prm, sh_, *reinterpret_cast<SeqScoreShared*>(reinterpret_cast<unsigned char*>(s_keys) + sco.lds_off),
                                         *reinterpret_cast<SeqSampleShared*>(reinterpret_cast<unsigned char*>(s_keys) + smp.lds_off), q, sco, smp.K, smp_cur, slot_key,
                                         drained || !stores_pending, as, n_tiles, sc_total, sc_nfit, sm_visited, pw, pn);
          if constexpr (NOM) {
            if (at != BS_INF && pn.own != kNmNone && t0) { nom.consumed[pn.own] = 1; nom.c_pod[pn.own] = i; nom.c_node[pn.own] = at; }
          }
          if (threadIdx.x == kSeqResultThread) { smp.start[i] = smp_cur; smp.visited[i] = sm_visited; }
          smp_cur = sample_step(smp_cur, sm_visited, N);     // (every wave holds the cursor: V is block-uniform)
        } else
        if constexpr (NOM) {
          // rule SP: rule S decides the candidates, rule P the choice among them (raw lanes, D8), D6 the consume behind it
          SeqPickNom pn{};
          pn.nom = &nom; pn.ns = ns; pn.prio = (int32_t)uni32((uint32_t)ns->pw_prio[pw]); pn.own = uni32(ns->pw_own[pw]);
          at = seq_pick_scored<TS, true>(nd, sq, prm, sh_, *reinterpret_cast<SeqScoreShared*>(reinterpret_cast<unsigned char*>(s_keys) + sco.lds_off), q, sco,
                                         slot_key, drained || !stores_pending, as, n_tiles, sc_total, sc_nfit, pw, pn);
          // consume (D6), no cursor to clear.  Thread 0's store is invisible to no later pod: every search reads consumed[] behind a
          // __syncthreads that follows this store — the one `stores_pending` asks for (set below by this very assume step) in front of the
          // next pod's scan, or else the one at the head of seq_pick_scored (`drained` false, stores_pending true).
          if (at != BS_INF && pn.own != kNmNone && t0) { nom.consumed[pn.own] = 1; nom.c_pod[pn.own] = i; nom.c_node[pn.own] = at; }
        } else {
        at = seq_pick_scored<TS>(nd, sq, prm, sh_, *reinterpret_cast<SeqScoreShared*>(reinterpret_cast<unsigned char*>(s_keys) + sco.lds_off), q, sco, slot_key,
                                 drained || !stores_pending, as, n_tiles, sc_total, sc_nfit, pw);
        }
        if (!drained) stores_pending = false;                // (the search drained them itself)
        if (threadIdx.x == kSeqResultThread) { sco.total[i] = sc_total; sco.n_fit[i] = sc_nfit; }
      } else {
      // first-fit cursor of the pod's request class (pods of a gang share a template: the search of the next one starts where this
      // one's ended).  Exact while (a) no assumed request has a negative lane — then free capacity only shrinks and a node that
      // could not hold this request cannot hold it later —, (b) the plugin's Filter does not gate the choice (its verdict moves
      // with the leader), (c) the cursor was left by the same fit class.
      // Under rule S (NOM), with rows that only TAKE room (the prologue switches the cursors off otherwise, through `mono`), the room a pod
      // sees grows with its priority and with every consumed row, so three more conditions: (d) an entry
      // remembers the priority Pc of the pod that left it and serves a pod only when P <= Pc (that pod sees every row the entry's pod saw);
      // (e) a pod with an own row neither reads nor writes a cursor (its own row is left out for it alone); (f) a consume clears every
      // entry (the row's room is free again for lower priorities); cursors written afterwards are valid again.
      SeqPickNom pn{};
      if constexpr (NOM) { pn.nom = &nom; pn.ns = ns; pn.prio = (int32_t)uni32((uint32_t)ns->pw_prio[pw]); pn.own = uni32(ns->pw_own[pw]); }
      bool cur_ok_;
      if constexpr (NOM) cur_ok_ = prm.use_cursor && mono && q.fl < 16u && q.fl != BS_FL_EVALUATED && q.pcls < nd.n_classes && pn.own == kNmNone;
      else cur_ok_ = prm.use_cursor && mono && q.fl < 16u && q.fl != BS_FL_EVALUATED && q.pcls < nd.n_classes;
      const bool cur_ok = cur_ok_;
      uint32_t pc = 0, ce = 0, start = 0;
      if (cur_ok) {
        pc = uni32(sh_.pw_pclass[pw]);
        ce = ((pc * 2654435761u) ^ (q.pcls * 40503u)) >> (32 - kSeqCursorBits);
        const unsigned long long cv = sh_.cur_kn[ce];
        if constexpr (NOM) {
          if ((uint32_t)(cv >> 32) == pc + 1u && sh_.cur_fc[ce] == q.pcls && (!nom.view || pn.prio <= ns->cur_prio[ce])) start = (uint32_t)cv;   // (no rows: every priority sees the same room)
        } else {
          if ((uint32_t)(cv >> 32) == pc + 1u && sh_.cur_fc[ce] == q.pcls) start = (uint32_t)cv;
        }
      }
      BS_SEQ_P(9);
      if (cur_ok && start >= nd.n) {
        at = BS_INF;                                         // an identical request found no node before, and nothing has been freed since
      } else {
        at = seq_pick<TS, NOM>(nd, sq, prm, sh_, q, slot_key, drained || !stores_pending, hit_par, as, n_tiles, start >> 6, pn);
        if (!drained) stores_pending = false;                // (the search drained them itself)
        if (cur_ok && t0) {                                  // (every wave read the entry before the search's barrier)
          sh_.cur_kn[ce] = ((unsigned long long)(pc + 1u) << 32) | (at != BS_INF ? at : nd.n);
          sh_.cur_fc[ce] = q.pcls;
          if constexpr (NOM) ns->cur_prio[ce] = pn.prio;
        }
      }
      if constexpr (NOM) {
        if (at != BS_INF && pn.own != kNmNone) {             // consume (D6): the row is dead for every later pod, whatever becomes of this one's gang
          if (t0) { nom.consumed[pn.own] = 1; nom.c_pod[pn.own] = i; nom.c_node[pn.own] = at; }
          for (uint32_t e = threadIdx.x; e < kSeqCursors; e += kSeqBlock) sh_.cur_kn[e] = 0ull;   // (f); ordered by the next pod's top barrier
        }
      }
      if (at != BS_INF) {
#pragma unroll
        for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
          if (j < L && j != 3 && q.preq[j] < 0 && (j < 3 || ((q.ppres >> (j - 4)) & 1u))) mono = false;   // capacity was FREED: cursors are history
      }
      }
      n_pick++;
      if (at != BS_INF) {
        stores_pending = true;
        // ---- the table summaries follow the assume step: the node's left values moved by the pod's request in every table the
        // node counts in (it is schedulable — no flag — so it is a row and has no taint error; what is left is the class's fit bit)
        if (!kLeanScored && prm.cache_slots) {
          int64_t dlt[BS_MAX_LANES];
          bool drop = false;                                 // a bound would break: negative request, or a scalar key the node's requests did not have
#pragma unroll
          for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
            dlt[j] = 0;
            if (j < L) {
              if (j < 3) dlt[j] = (j == BS_LANE_EPH && !gate) ? 0 : q.preq[j];
              else if (j == 3) dlt[j] = 1;
              else if ((q.ppres >> (j - 4)) & 1u) {
                if (!((as.ap >> (j - 4)) & 1u)) dlt[j] = 0;                        // allocatable lacks the key: the lane never exists for this node
                else if ((as.rp >> (j - 4)) & 1u) dlt[j] = q.preq[j];
                else drop = true;                                                  // the lane starts to exist at this node
              }
              if (dlt[j] < 0) drop = true;
            }
          }
          const uint32_t ta = at >> 6;
#pragma unroll
          for (uint32_t c = 0; c < kSeqCacheSlots; ++c) {
            if (c < prm.cache_slots && slot_key[c] != BS_INF && ((as.fitbits >> c) & 1u)) {
              if (drop) slot_key[c] = BS_INF;                // summarised afresh at its next use
              else {
                for (uint32_t t = ta + threadIdx.x; t < ch.T; t += kSeqBlock) {       // the node's tile (its total) and every tile behind it (their offsets)
                  unsigned long long* pb = (t == ta ? ch.tt : ch.off) + (size_t)c * L * ch.T + t;
                  unsigned long long cur[BS_MAX_LANES];      // every lane's word fetched before the first is written back (one LDS latency, not L)
#pragma unroll
                  for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
                    if (j < L) cur[j] = pb[(size_t)j * ch.T];
#pragma unroll
                  for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
                    if (j < L) pb[(size_t)j * ch.T] = cur[j] - (unsigned long long)dlt[j];
                }
              }
            }
          }
        }
      }
    }
    BS_SEQ_T(4);
    BS_SEQ_P(14);
    if (deny) { gflags |= BS_GROUP_DENIED; own.flags = gflags; }
    if (threadIdx.x == kSeqResultThread) {                  // write-only results: not wave 0, whose thread 0 has the group and node bookkeeping to do
      sq.pf_code[i] = (uint8_t)code;
      if (sq.pf_first_k) sq.pf_first_k[i] = fk;
      if (sq.pf_leader) sq.pf_leader[i] = sop_leader;
    }
    if (t0 && deny) sq.g_flags[gi] = (uint8_t)gflags;
    BS_SEQ_P(15);
    if (at != BS_INF && !grouped) {                          // core.go:269-272: Permit lets it through at once
      if (t0) sq.pod_node[i] = (int32_t)at;
    } else if (at != BS_INF) {
      // ---- Permit, core.go:268-309.  Every wave applies the update to its copy of the group; thread 0 writes it out.
      const uint32_t mm = pod_mm;
      const uint32_t m1 = gmatched + 1u;                                                             // :290
      const bool ready = m1 >= (uint32_t)(mm - gsc);                                                 // :303
      // sendStartScheduleSignal -> StartBatchSchedule (batchscheduler.go:254-344) releases — unless the phase is none of PreScheduling /
      // Scheduling (:258-261): then the latch is all that happens and the pod waits on like any other
      const bool release = ready && !(gflags & BS_GROUP_PHASE_CLOSED);
      const uint32_t has_rec = own.nwait & kSeqHasRecord, nw = own.nwait & ~kSeqHasRecord;
      const uint32_t prev = own.head, k = nw + 1u;
      if (ready) gflags |= BS_GROUP_SCHEDULED_LATCH;                                                 // :305
      if (!release) {
        if (t0) {
          sq.g_matched[gi] = m1;
          if (gflags != own.flags) sq.g_flags[gi] = (uint8_t)gflags;
          sq.wait_rec[i] = ((unsigned long long)prev << 32) | at;
          sq.head[gi] = i + 1u;
          sq.nwait[gi] = k | has_rec;
          if (wl_ok && wl_cnt < kSeqWaitList) { sh_.wl_pod[wl_cnt] = i; sh_.wl_node[wl_cnt] = at; }
        }
        own.matched = m1;
        own.flags = gflags;
        own.head = i + 1u;
        own.nwait = k | has_rec;
        if (wl_cnt < kSeqWaitList) wl_cnt++; else wl_ok = false;
      } else {
        // EVERY entry of MatchedPodNodes is allowed (:292,:301-333), deleted (:326) and counted by PostBind (core.go:327): the pods this
        // pass placed — they bind in parallel from the LDS list when it holds them all — and the m1 - k that were waiting when it began
        const bool from_list = wl_ok && wl_cnt == nw;
        if (from_list) {
          for (uint32_t e = threadIdx.x; e < wl_cnt; e += kSeqBlock) sq.pod_node[sh_.wl_pod[e]] = (int32_t)sh_.wl_node[e];
        }
        const uint32_t scn = gsc + m1;                                                               // PostBind, core.go:327 (uint32)
        if (scn >= mm) gflags |= BS_GROUP_PHASE_CLOSED;                                              // core.go:329-330 phase Scheduled
        if (t0) {
          sq.g_matched[gi] = 0;
          sq.pod_node[i] = (int32_t)at;
          if (!from_list)
            for (uint32_t wv = prev; wv != 0u;) {
              const unsigned long long rec = sq.wait_rec[wv - 1u];
              sq.pod_node[wv - 1u] = (int32_t)(uint32_t)rec;
              wv = (uint32_t)(rec >> 32);
            }
          sq.head[gi] = 0;
          sq.nwait[gi] = kSeqHasRecord;
          sq.g_sc[gi] = scn;
          sq.g_flags[gi] = (uint8_t)gflags;
          if (!has_rec) {
            if (n_released < sq.cap) {
              sq.released_group[n_released] = (uint32_t)gi;
              sq.released_pods[n_released] = m1;
              sq.first_tick[n_released] = sq.t_first[gi];
              sq.ready_tick[n_released] = (unsigned long long)wall_clock64() - clk0;
              sq.slot_of[gi] = n_released;
            }
          } else if (sq.slot_of[gi] != BS_INF) {
            sq.released_pods[sq.slot_of[gi]] += m1;          // a second release of the gang (Status.Scheduled still below MinMember: only through uint32 wrap)
          }
        }
        own.matched = 0;
        own.head = 0;
        own.nwait = kSeqHasRecord;
        own.sc = scn;
        own.flags = gflags;
        wl_cnt = 0;
        wl_ok = true;
        if (!has_rec) n_released++;
      }
      {
        // matched moved: the group's progress changed.  findMaxPG's answer stands unless this key now beats the winner's, or the
        // winner itself fell back (released: no candidate any more).
        const unsigned long long key = seq_key((uint32_t)gi, own.flags, mm, own.sc, own.matched);
        if (t0) { if (prm.keys_in_lds) s_keys[gi] = key; else sq.keys[gi] = key; }
        if (fold_valid) {
          if (fold_top == 0ull || fold_panic) fold_valid = false;
          else if (gi == fold_leader) { if (key < fold_top || (key & 1ull) || key == ~0ull) fold_valid = false; else fold_top = key; }
          else if (key > fold_top) fold_valid = false;
        }
      }
    }
    if (grouped && gi == ldr_of) {                           // the leader's copy follows what this pod did to its group
      const uint32_t h = ldr.head;
      ldr = own;
      ldr.head = h;
    }
    BS_SEQ_T(5);
    BS_SEQ_P(16);
  }
  BS_SEQ_FULL_BARRIER();
  if constexpr (SAMPLE) {
    if (threadIdx.x == kSeqResultThread) smp.next[0] = smp_cur;      // the cursor behind the last pod: the caller hands it to the next pass
  }
  if (t0) {
    sq.info[0] = n_released;
    sq.info[1] = (unsigned long long)wall_clock64() - clk0;
    sq.info[2] = n_pick;
    sq.info[3] = n_scan;
    sq.info[4] = (unsigned long long)(uint32_t)(sop_leader + 1);
    sq.info[5] = n_rounds;
    sq.info[6] = n_tiles;
    sq.info[7] = n_folds | (n_builds << 40);
#ifdef BS_SEQ_PROBE
    for (int k = 0; k < 8; ++k) sq.info[8 + k] = ph[k];
    for (int k = 0; k < 8; ++k) { sq.info[16 + k] = g_seq_scan_ph[k]; g_seq_scan_ph[k] = 0; }
    for (int k = 0; k < 32; ++k) sq.info[32 + k] = sh_.ph2[k];
#endif
  }
