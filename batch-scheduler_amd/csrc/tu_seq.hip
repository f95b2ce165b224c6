// tu_seq.hip — translation unit of the sequential pass: its kernel (bs_seq.hpp: k_seq_pass<TS>, six instantiations; k_seq_pass<TS, true>, the
// same six under rule S, are emitted by tu_seq_nom.hip, k_seq_scored<TS>, the thirteen under rule P, by tu_seq_score.hip, k_seq_sp<TS>,
// the thirteen under rule SP, by tu_seq_score_nom.hip, k_seq_sampled<TS> and k_seq_sampled_nom<TS>, the two families under rule F, by
// tu_seq_sample.hip and tu_seq_sample_nom.hip), the file-local launch wrapper and the entry points bs_seq_run, bs_seq_run_nominated,
// bs_seq_run_scored, bs_seq_run_scored_nominated and the two sampled forms (include/bsched.h) with their flat forms,
// bs_seq_nominated_read, bs_seq_score_read and bs_seq_sample_read; see tu_fast.hip for why.  The nominated-pod table is reached through bs_ctx.hpp's declarations
// (tu_nominated.hip defines them): this unit does not include bs_nominated.hpp and emits no k_nm_* kernel.
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bs_seq.hpp"
#include "bs_ctx.hpp"
#include "bs_nominated_check.hpp"

namespace bs {

static void launch_seq(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq, const SeqParams& prm) {
  lanes_narrow(S, [&](auto s) {
    constexpr int TS = decltype(s)::value;
    // static LDS (first-fit bounds, reduction slots) + the key window can exceed the default 64 KB of dynamic LDS
    void (*kn)(PodsDev, GroupsDev, NodesDev, SeqDev, SeqParams) = &k_seq_pass<TS>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seq_pass<TS>), dim3(1), dim3(kSeqBlock), lds, stream, pd, gr, nd, sq, prm);
  });
}

// what bs_seq_run_nominated hands the pass: the caller's priorities and, per pod, the ROW of its own nomination (kNmNone: none)
struct SeqNomCall {
  const int32_t* priority;
  const std::vector<uint32_t>* own_row;
};

// what both entry points refuse on the host before anything else
static int seq_refusals(bs_ctx* c, uint32_t stages) {
  if (!c->have_nodes || !c->have_fit || !c->have_groups || !c->have_pods) {
    c->last_error = "bs_seq_run needs nodes, fit, groups and pods loaded";
    return BS_ERR_STATE;
  }
  if (!(stages & BS_STAGE_PREFILTER)) { c->last_error = "PREFILTER stage is mandatory"; return BS_ERR_INVALID; }
  if ((stages & BS_BATCH_FILTER_DENY) && !(stages & BS_STAGE_FILTER)) { c->last_error = "BS_BATCH_FILTER_DENY needs BS_STAGE_FILTER"; return BS_ERR_INVALID; }
  if (c->nranks > 1 || c->reduce_external) { c->last_error = "bs_seq_run is single-rank only (a sequential pass does not shard)"; return BS_ERR_STATE; }
  return BS_OK;
}

}  // namespace bs

// bs_seq_run's body behind the refusals above; nc: null = no table (bs_seq_run), else rule S; score: null = first fit, else rule P; sample (with
// score only): null = the full search, else rule F
static int seq_run_impl(bs_ctx* c, uint32_t stages, bs_seq_out* out, const SeqNomCall* nc, const bs_seq_score* score = nullptr,
                        const bs_seq_sample* sample = nullptr) {
  int rc = use_device(c);
  if (rc) return rc;
  if ((rc = settle_pending(c))) return rc;
  const uint32_t P = c->P, G = c->G, N = c->N, C = c->C, L = c->L;
  if ((G > c->n_uncaptured && c->max_group_cls >= C) || (P && c->max_pod_cls >= C)) {
    c->last_error = "fit class index out of range (groups.cls / pods.cls vs the loaded fit classes)";
    return BS_ERR_INVALID;
  }
  if (G > 0x7FFFFFF0u) return BS_ERR_CAPACITY;
  c->seq_wait_valid = false;                                // the pass replaces the waiting state
  c->seq_nom_valid = false;                                 // ... and is the context's last pass
  c->seq_score_valid = false;
  c->seq_sample_valid = false;
  // the first-fit cursors are keyed by the resident queue's request classes: a queue patch whose insert wave ran out of class ids
  // (kHiIdOverflow of h_info, set by the device) left them unusable until the queue is re-derived — check_handover does that
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // An unread batch's error words are looked at here (the id overflow concerns this pass: check_handover re-derives the queue) but they stay
  // that batch's: batch_void keeps every later read of it failing with BS_ERR_RETRY until bs_batch_run starts a new one.  The pass itself
  // reads no batch result and goes on.
  if ((rc = check_handover(c)) && rc != BS_ERR_RETRY) return rc;
  if (rc == BS_ERR_RETRY) c->last_error.clear();            // (nothing failed for THIS call)
  out->n_released = 0;
  out->total_ns = 0;
  out->node_picks = out->node_scans = out->scan_rounds = out->pick_rounds = out->leader_folds = out->table_builds = 0;
  // ---- scratch: one allocation
  const size_t nP = std::max<uint32_t>(P, 1), nG = std::max<uint32_t>(G, 1), cap = std::max<uint32_t>(out->cap, 1), stride = std::max<uint32_t>(c->Ncap, 1);
  Carve cv;
  const auto o_sc07 = cv.take<int64_t>(stride * L);
  const auto o_sc10 = cv.take<int64_t>(stride * L);
  const auto o_meta = cv.take<uint32_t>(stride);
  const auto o_keys = cv.take<unsigned long long>(nG);
  const auto o_wait = cv.take<unsigned long long>(nP);
  const auto o_head = cv.take<uint32_t>(nG);
  const auto o_nwait = cv.take<uint32_t>(nG);
  const auto o_slot = cv.take<uint32_t>(nG);
  const auto o_tfirst = cv.take<unsigned long long>(nG);
  const size_t o_res = cv.mark();                           // results: one D2H
  const auto o_code = cv.take<uint8_t>(nP);
  const auto o_node = cv.take<int32_t>(nP);
  const auto o_fk = cv.take<uint32_t>(nP);
  const auto o_leader = cv.take<int32_t>(nP);
  const auto o_lperm = cv.take<uint8_t>(nP);
  const auto o_rg = cv.take<uint32_t>(cap);
  const auto o_rp = cv.take<uint32_t>(cap);
  const auto o_ft = cv.take<unsigned long long>(cap);
  const auto o_rt = cv.take<unsigned long long>(cap);
  const auto o_info = cv.take<unsigned long long>(64);
  // rule S: the consumed bytes and the per-row result words ride the result block; the call's two per-pod arrays are one H2D block
  const uint32_t W = nc ? c->nom_w : 0u;
  const auto o_cflag = cv.take<uint8_t>(nc ? std::max<uint32_t>(W, 1) : 0);
  const auto o_cpod = cv.take<uint32_t>(nc ? std::max<uint32_t>(W, 1) : 0);
  const auto o_cnode = cv.take<uint32_t>(nc ? std::max<uint32_t>(W, 1) : 0);
  const size_t o_res_end = cv.mark();
  const auto o_pin = cv.take<uint32_t>(nc ? 2 * nP : 0);    // priority[P], own_row[P]
  HIPCHK(c, c->d_seq.reserve(cv.mark()));
  uint8_t* base = c->d_seq.as<uint8_t>();
  GroupsDev gr = groups_dev(c);
  SeqDev sq{};
  sq.nreq = c->d_nreq.as<int64_t>();
  sq.rpres = c->d_rpres.as<uint32_t>();
  sq.g_matched = const_cast<uint32_t*>(gr.matched);
  sq.g_sc = const_cast<uint32_t*>(gr.status_scheduled);
  sq.g_flags = const_cast<uint8_t*>(gr.flags);
  sq.g_cls = const_cast<uint32_t*>(gr.cls);
  sq.g_minres = const_cast<int64_t*>(gr.minres);
  sq.g_mrpres = const_cast<uint32_t*>(gr.mrpres);
  sq.g_occ = const_cast<uint64_t*>(gr.occupied);
  sq.left07 = o_sc07.in(base);
  sq.left10 = o_sc10.in(base);
  sq.nmeta = o_meta.in(base);
  sq.keys = o_keys.in(base);
  sq.wait_rec = o_wait.in(base);
  sq.head = o_head.in(base);
  sq.nwait = o_nwait.in(base);
  sq.slot_of = o_slot.in(base);
  sq.t_first = o_tfirst.in(base);
  sq.pclass = pclass_dev(c);
  sq.pf_code = o_code.in(base);
  sq.pod_node = o_node.in(base);
  sq.pf_first_k = o_fk.in(base);
  sq.pf_leader = o_leader.in(base);
  sq.last_permitted = o_lperm.in(base);
  sq.released_group = o_rg.in(base);
  sq.released_pods = o_rp.in(base);
  sq.first_tick = o_ft.in(base);
  sq.ready_tick = o_rt.in(base);
  sq.cap = out->cap;
  sq.info = o_info.in(base);
  SeqParams prm{};
  prm.S = c->S;
  prm.eph_gate = c->cfg.eph_gate;
  prm.run_filter = (stages & BS_STAGE_FILTER) ? 1u : 0u;
  prm.filter_deny = (stages & BS_BATCH_FILTER_DENY) ? 1u : 0u;
  prm.C = C;
  prm.sop_leader0 = c->sop_leader0;
  prm.keys_in_lds = G <= kSeqKeysLds ? 1u : 0u;
  prm.prune = cdiv(N, 64) <= kSeqPruneTiles ? 1u : 0u;
  size_t lds = prm.keys_in_lds ? align256((size_t)nG * 8) : 0;
  {
    // table summaries: as many slots as the CU's LDS holds behind the static arrays and the key window (one thread per tile: <= 1024 tiles)
    const size_t T = cdiv(N, 64), per_slot = T * ((size_t)L * 24 + 8), query = 0;
    const size_t budget = (size_t)160 * 1024 - sizeof(SeqShared) - 2048 - (nc ? align256(sizeof(SeqNomShared)) : 0) - (score ? align256(sizeof(SeqScoreShared)) : 0) -
                          (sample ? align256(sizeof(SeqSampleShared)) : 0);
    uint32_t K = 0;
    if (T && T <= (size_t)kSeqPruneTiles && budget > lds + query + per_slot) K = (uint32_t)std::min<size_t>(kSeqCacheSlots, (budget - lds - query) / per_slot);
    if (score && c->S > (uint32_t)kSeqScoredFullLanes) K = 0;   // (the lean scored kernels keep no table summaries: bs_seq_pass.inc)
    if (const char* e = std::getenv("BS_SEQ_CACHE_SLOTS")) K = std::min<uint32_t>(K, (uint32_t)std::max(0, std::atoi(e)));   // tests: 0 = the round scan, 1 = thrash one slot
    prm.cache_slots = K;
    prm.cache_off = (uint32_t)lds;
    if (K) lds += align256(K * per_slot + query + 64);
  }
  // first-fit cursors per request class (bs_seq.hpp, seq_pick): BS_SEQ_NO_CURSOR=1 = every search starts at the head of the list
  prm.use_cursor = (P && sq.pclass && !(std::getenv("BS_SEQ_NO_CURSOR") && std::atoi(std::getenv("BS_SEQ_NO_CURSOR")))) ? 1u : 0u;
  HIPCHK(c, hipMemsetAsync(o_info.in(base), 0, o_info.bytes(), c->stream));
  SeqNom nom{};
  std::vector<uint32_t> pin;
  if (nc) {
    nom.view = nom_view(c);
    nom.rows = W;
    nom.consumed = o_cflag.in(base);
    nom.c_pod = o_cpod.in(base);
    nom.c_node = o_cnode.in(base);
    nom.pprio = reinterpret_cast<const int32_t*>(o_pin.in(base));
    nom.pown = o_pin.in(base) + nP;
    nom.lds_off = (uint32_t)lds;
    lds += align256(sizeof(SeqNomShared));
    pin.assign(2 * nP, kNmNone);
    if (P) {
      std::memcpy(pin.data(), nc->priority, (size_t)P * 4);
      std::memcpy(pin.data() + nP, nc->own_row->data(), (size_t)P * 4);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (nothing of an earlier call still reads the block)
    HIPCHK(c, hipMemcpy(o_pin.in(base), pin.data(), o_pin.bytes(), hipMemcpyHostToDevice));   // synchronous: pin is a local buffer and a later error returns at once
    HIPCHK(c, hipMemsetAsync(o_cflag.in(base), 0, o_cflag.bytes(), c->stream));
  }
  SeqScore sco{};
  if (score) {
    // rule P: the weights, the two per-pod result arrays (context-owned, sized with the queue, zero where the choice is not reached)
    HIPCHK(c, c->d_seq_score.reserve(2 * nP * sizeof(uint32_t)));
    HIPCHK(c, hipMemsetAsync(c->d_seq_score.p, 0, 2 * nP * sizeof(uint32_t), c->stream));
    sco.w_least = score->w_least; sco.w_most = score->w_most; sco.w_balanced = score->w_balanced;
    sco.total = c->d_seq_score.as<uint32_t>();
    sco.n_fit = sco.total + nP;
    sco.lds_off = (uint32_t)lds;
    lds += align256(sizeof(SeqScoreShared));
  }
  SeqSample smp{};
  if (sample) {
    // rule F: K and the first cursor, normalised; the two per-pod result arrays and the cursor behind the last pod (context-owned, zero
    // where the choice is not reached)
    const size_t words = 2 * nP + 1;
    HIPCHK(c, c->d_seq_sample.reserve(words * sizeof(uint32_t)));
    HIPCHK(c, hipMemsetAsync(c->d_seq_sample.p, 0, words * sizeof(uint32_t), c->stream));
    smp.K = sample_k(sample->num_to_find, N);
    smp.s0 = sample_start(sample->start, N);
    smp.start = c->d_seq_sample.as<uint32_t>();
    smp.visited = smp.start + nP;
    smp.next = smp.start + 2 * nP;
    smp.lds_off = (uint32_t)lds;
    lds += align256(sizeof(SeqSampleShared));
  }
  const PodsDev pd = pods_dev(c);
  const NodesDev nd = nodes_dev(c);
  if (sample && nc) launch_seq_sampled_nominated(c->stream, c->S, lds, pd, gr, nd, sq, prm, nom, sco, smp);   // (tu_seq_sample_nom.hip: rule F over rule SP)
  else if (sample) launch_seq_sampled(c->stream, c->S, lds, pd, gr, nd, sq, prm, sco, smp);   // (tu_seq_sample.hip: rule F over rule P)
  else if (score && nc) launch_seq_scored_nominated(c->stream, c->S, lds, pd, gr, nd, sq, prm, nom, sco);   // (tu_seq_score_nom.hip: rule SP)
  else if (score) launch_seq_scored(c->stream, c->S, lds, pd, gr, nd, sq, prm, sco);   // (tu_seq_score.hip: the scored instantiations)
  else if (nc) launch_seq_nominated(c->stream, c->S, lds, pd, gr, nd, sq, prm, nom);   // (tu_seq_nom.hip: the NOM instantiations)
  else launch_seq(c->stream, c->S, lds, pd, gr, nd, sq, prm);
  LAUNCHCHK(c, BS_KERNEL_QUERY);
  // ---- results: one copy of the whole result block, then the caller's arrays
  std::vector<uint8_t> res(o_res_end - o_res);
  HIPCHK(c, hipMemcpyAsync(res.data(), base + o_res, res.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* rb = res.data() - o_res;
  const unsigned long long* info = o_info.in(rb);
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device) != hipSuccess || khz <= 0) khz = 100000;   // 100 MHz
  auto to_ns = [&](unsigned long long ticks) { return (int64_t)((long double)ticks * 1.0e6L / (long double)khz); };
  out->n_released = (uint32_t)info[0];
  out->total_ns = to_ns(info[1]);
  out->node_picks = info[2];
  out->node_scans = info[3];
  out->scan_rounds = info[5];
  out->pick_rounds = info[6];
  out->leader_folds = info[7] & ((1ull << 40) - 1ull);
  out->table_builds = info[7] >> 40;
  if (const char* e = std::getenv("BS_SEQ_PROBE_PRINT")) {   // probe build: cycles per phase (see bs_seq.hpp)
    if (std::atoi(e)) std::fprintf(stderr, "seq probe cycles: control %llu capture %llu fold %llu scan %llu pick %llu permit %llu top-barrier %llu\n", info[8], info[9],
                                   info[10], info[11], info[12], info[13], info[14]);
    if (std::atoi(e)) std::fprintf(stderr, "  scan rounds (thread 0): issue-next-loads %llu select %llu wave-scans %llu lds-writes %llu barrier %llu fk-check %llu offsets+compare %llu tail %llu\n",
                                   info[16], info[17], info[18], info[19], info[20], info[21], info[22], info[23]);
    if (std::atoi(e)) {                                      // the finer split of thread 0's time (BS_SEQ_P in bs_seq.hpp)
      static const char* nm[17] = {"top-barrier", "group-loads", "control", "scan:drain", "scan:slot", "scan:candidates", "scan:tiles", "scan:barrier+min", "scan:tail",
                                   "pick:request", "pick:drain", "pick:tiles", "pick:barrier+min", "pick:assume", "summaries", "result-stores", "permit"};
      std::fprintf(stderr, "  thread 0, cycles:");
      for (int k2 = 0; k2 < 17; ++k2) std::fprintf(stderr, " %s %llu |", nm[k2], info[32 + k2]);
      std::fprintf(stderr, "\n");
    }
  }
  if (P) {
    if (out->pf_code) std::memcpy(out->pf_code, o_code.in(rb), P);
    if (out->pod_node) std::memcpy(out->pod_node, o_node.in(rb), (size_t)P * 4);
    if (out->pf_first_k) std::memcpy(out->pf_first_k, o_fk.in(rb), (size_t)P * 4);
    if (out->pf_leader) std::memcpy(out->pf_leader, o_leader.in(rb), (size_t)P * 4);
    if (out->last_permitted) { if (prm.filter_deny) std::memcpy(out->last_permitted, o_lperm.in(rb), P); else std::memset(out->last_permitted, 0, P); }
    c->sop_leader0 = (int32_t)(uint32_t)info[4] - 1;         // sop.maxFinishedPG as the pass left it
  }
  const uint32_t k = std::min(out->n_released, out->cap);
  if (k) {
    if (out->released_group) std::memcpy(out->released_group, o_rg.in(rb), (size_t)k * 4);
    if (out->released_pods) std::memcpy(out->released_pods, o_rp.in(rb), (size_t)k * 4);
    const unsigned long long* ft = o_ft.in(rb);
    const unsigned long long* rt = o_rt.in(rb);
    for (uint32_t i = 0; i < k; ++i) {
      if (out->first_ns) out->first_ns[i] = to_ns(ft[i]);
      if (out->ready_ns) out->ready_ns[i] = to_ns(rt[i]);
    }
  }
  // ---- the host mirrors and everything derived from the state the pass rewrote
  if (N && P) {
    HIPCHK(c, hipMemcpy2D(c->h_nreq.data(), (size_t)N * 8, c->d_nreq.p, (size_t)c->Ncap * 8, (size_t)N * 8, L, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(c->h_rpres.data(), c->d_rpres.p, (size_t)N * 4, hipMemcpyDeviceToHost));
    rederive_nodes(c);   // left4 / cluster bounds follow the requests (flags, hence kmap, are unchanged)
    LAUNCHCHK(c, BS_KERNEL_PREPASS);
  }
  c->bitmap_valid = false;
  if (G && P) {
    std::vector<uint32_t> cls(G);
    HIPCHK(c, hipMemcpy(c->h_gflags.data(), gr.flags, G, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(cls.data(), gr.cls, (size_t)G * 4, hipMemcpyDeviceToHost));
    c->n_uncaptured = 0;
    c->n_nominres = 0;
    c->max_group_cls = 0;
    for (uint32_t i = 0; i < G; ++i) {
      if (!(c->h_gflags[i] & BS_GROUP_HAS_POD)) c->n_uncaptured++;
      else c->max_group_cls = std::max(c->max_group_cls, cls[i]);
      if (!(c->h_gflags[i] & BS_GROUP_HAS_MINRES)) c->n_nominres++;
    }
    if ((rc = analyse_groups(c))) return rc;
    if ((rc = maybe_analyse_epochs(c))) return rc;
  }
  if (nc) {
    // ---- consume (D6): the rows whose pods were assumed leave the table by the stable compaction; their ids are dead
    const uint8_t* cf = o_cflag.in(rb);
    const uint32_t* cp = o_cpod.in(rb);
    const uint32_t* cn = o_cnode.in(rb);
    std::vector<uint32_t> id, pod, node;
    for (uint32_t r = 0; r < W; ++r)
      if (cf[r]) { id.push_back(c->nom_live[r]); pod.push_back(cp[r]); node.push_back(cn[r]); }
    if ((rc = nom_drop_flagged(c, o_cflag.in(base), id))) return rc;
    c->seq_nom_id.swap(id);
    c->seq_nom_pod.swap(pod);
    c->seq_nom_node.swap(node);
    c->seq_nom_valid = true;
  }
  c->seq_o_wait = o_wait;                                  // (the pieces: seq_expire_dev addresses them in d_seq)
  c->seq_o_head = o_head;
  c->seq_o_nwait = o_nwait;
  c->seq_o_node = o_node;
  c->seq_wait_valid = true;
  if (score) { c->seq_score_p = P; c->seq_score_valid = true; }
  if (sample) c->seq_sample_valid = true;
  return BS_OK;
}

extern "C" {
int bs_seq_run(bs_ctx* c, uint32_t stages, bs_seq_out* out) {
  if (!c || !out) return BS_ERR_INVALID;
  if (const int rc = seq_refusals(c, stages)) return rc;
  return seq_run_impl(c, stages, out, nullptr);
}

int bs_seq_run_nominated(bs_ctx* c, uint32_t stages, uint32_t p, const int32_t* priority, const uint32_t* own_id, bs_seq_out* out) {
  if (!c || !out) return BS_ERR_INVALID;
  if (const int rc = seq_refusals(c, stages)) return rc;
  if (stages & BS_STAGE_FILTER) {
    c->last_error = "bs_seq_run_nominated: BS_STAGE_FILTER is refused (the plugin's Filter takes no part in the fit test under nominees, as in bs_preempt_run)";
    return BS_ERR_INVALID;
  }
  if (p != c->P) { c->last_error = "bs_seq_run_nominated: p is not the resident queue's length (bs_pods_count)"; return BS_ERR_INVALID; }
  if (p && !priority) { c->last_error = "bs_seq_run_nominated: priority is NULL and the queue has pods"; return BS_ERR_INVALID; }
  if (const int rc = nom_state(c, "bs_seq_run_nominated")) return rc;
  std::vector<uint32_t> own_row;
  if (const int bad = nom_own_check(c->nom_live.data(), c->nom_w, c->nom_ids, p, own_id, BS_NOM_NONE, own_row)) {
    c->last_error = std::string("bs_seq_run_nominated: ") + nom_own_check_text(bad);
    return BS_ERR_INVALID;
  }
  static_assert(BS_NOM_NONE == kNmNone, "an own id of BS_NOM_NONE becomes the row index the kernel skips nothing for");
  const SeqNomCall nc{priority, &own_row};
  return seq_run_impl(c, stages, out, &nc);
}

int bs_seq_run_scored(bs_ctx* c, uint32_t stages, const bs_seq_score* score, bs_seq_out* out) {
  if (!c || !out) return BS_ERR_INVALID;
  if (const int rc = seq_refusals(c, stages)) return rc;
  if (!score) { c->last_error = "bs_seq_run_scored: score is NULL"; return BS_ERR_INVALID; }
  static_assert(BS_SCORE_WEIGHT_MAX == kScoreWeightMax, "the header's bound is the one bs_seq_score.hpp's total rests on");
  if (score->w_least > BS_SCORE_WEIGHT_MAX || score->w_most > BS_SCORE_WEIGHT_MAX || score->w_balanced > BS_SCORE_WEIGHT_MAX) {
    c->last_error = "bs_seq_run_scored: a weight is above BS_SCORE_WEIGHT_MAX";
    return BS_ERR_INVALID;
  }
  return seq_run_impl(c, stages, out, nullptr, score);
}

int bs_seq_run_scored_nominated(bs_ctx* c, uint32_t stages, uint32_t p, const int32_t* priority, const uint32_t* own_id, const bs_seq_score* score,
                                bs_seq_out* out) {
  // the refusals of bs_seq_run_nominated in its order, then those of bs_seq_run_scored: all before any launch, nothing resident changes
  if (!c || !out) return BS_ERR_INVALID;
  if (const int rc = seq_refusals(c, stages)) return rc;
  if (stages & BS_STAGE_FILTER) {
    c->last_error = "bs_seq_run_scored_nominated: BS_STAGE_FILTER is refused (the plugin's Filter takes no part in the fit test under nominees, as in bs_preempt_run)";
    return BS_ERR_INVALID;
  }
  if (p != c->P) { c->last_error = "bs_seq_run_scored_nominated: p is not the resident queue's length (bs_pods_count)"; return BS_ERR_INVALID; }
  if (p && !priority) { c->last_error = "bs_seq_run_scored_nominated: priority is NULL and the queue has pods"; return BS_ERR_INVALID; }
  if (const int rc = nom_state(c, "bs_seq_run_scored_nominated")) return rc;
  std::vector<uint32_t> own_row;
  if (const int bad = nom_own_check(c->nom_live.data(), c->nom_w, c->nom_ids, p, own_id, BS_NOM_NONE, own_row)) {
    c->last_error = std::string("bs_seq_run_scored_nominated: ") + nom_own_check_text(bad);
    return BS_ERR_INVALID;
  }
  if (!score) { c->last_error = "bs_seq_run_scored_nominated: score is NULL"; return BS_ERR_INVALID; }
  if (score->w_least > BS_SCORE_WEIGHT_MAX || score->w_most > BS_SCORE_WEIGHT_MAX || score->w_balanced > BS_SCORE_WEIGHT_MAX) {
    c->last_error = "bs_seq_run_scored_nominated: a weight is above BS_SCORE_WEIGHT_MAX";
    return BS_ERR_INVALID;
  }
  const SeqNomCall nc{priority, &own_row};
  return seq_run_impl(c, stages, out, &nc, score);
}

// what both sampled forms refuse behind their parents' refusals
static int seq_sample_refusals(bs_ctx* c, uint32_t stages, const bs_seq_sample* sample, const char* who) {
  if (!sample) { c->last_error = std::string(who) + ": sample is NULL"; return BS_ERR_INVALID; }
  if (stages & BS_BATCH_FILTER_DENY) {
    c->last_error = std::string(who) + ": BS_BATCH_FILTER_DENY is refused (Filter's TTL writes are defined over every node offered; a sampled walk offers the visited nodes only)";
    return BS_ERR_INVALID;
  }
  return BS_OK;
}

uint32_t bs_seq_sample_size(uint32_t n, int32_t percentage) { return sample_size(n, percentage); }

int bs_seq_run_scored_sampled(bs_ctx* c, uint32_t stages, const bs_seq_score* score, const bs_seq_sample* sample, bs_seq_out* out) {
  // the refusals of bs_seq_run_scored in its order, then the sampled form's own: all before any launch, nothing resident changes
  if (!c || !out) return BS_ERR_INVALID;
  if (const int rc = seq_refusals(c, stages)) return rc;
  if (!score) { c->last_error = "bs_seq_run_scored_sampled: score is NULL"; return BS_ERR_INVALID; }
  if (score->w_least > BS_SCORE_WEIGHT_MAX || score->w_most > BS_SCORE_WEIGHT_MAX || score->w_balanced > BS_SCORE_WEIGHT_MAX) {
    c->last_error = "bs_seq_run_scored_sampled: a weight is above BS_SCORE_WEIGHT_MAX";
    return BS_ERR_INVALID;
  }
  if (const int rc = seq_sample_refusals(c, stages, sample, "bs_seq_run_scored_sampled")) return rc;
  return seq_run_impl(c, stages, out, nullptr, score, sample);
}

int bs_seq_run_scored_nominated_sampled(bs_ctx* c, uint32_t stages, uint32_t p, const int32_t* priority, const uint32_t* own_id, const bs_seq_score* score,
                                        const bs_seq_sample* sample, bs_seq_out* out) {
  // the refusals of bs_seq_run_scored_nominated in its order, then the sampled form's own
  if (!c || !out) return BS_ERR_INVALID;
  if (const int rc = seq_refusals(c, stages)) return rc;
  if (stages & BS_STAGE_FILTER) {
    c->last_error = "bs_seq_run_scored_nominated_sampled: BS_STAGE_FILTER is refused (the plugin's Filter takes no part in the fit test under nominees, as in bs_preempt_run)";
    return BS_ERR_INVALID;
  }
  if (p != c->P) { c->last_error = "bs_seq_run_scored_nominated_sampled: p is not the resident queue's length (bs_pods_count)"; return BS_ERR_INVALID; }
  if (p && !priority) { c->last_error = "bs_seq_run_scored_nominated_sampled: priority is NULL and the queue has pods"; return BS_ERR_INVALID; }
  if (const int rc = nom_state(c, "bs_seq_run_scored_nominated_sampled")) return rc;
  std::vector<uint32_t> own_row;
  if (const int bad = nom_own_check(c->nom_live.data(), c->nom_w, c->nom_ids, p, own_id, BS_NOM_NONE, own_row)) {
    c->last_error = std::string("bs_seq_run_scored_nominated_sampled: ") + nom_own_check_text(bad);
    return BS_ERR_INVALID;
  }
  if (!score) { c->last_error = "bs_seq_run_scored_nominated_sampled: score is NULL"; return BS_ERR_INVALID; }
  if (score->w_least > BS_SCORE_WEIGHT_MAX || score->w_most > BS_SCORE_WEIGHT_MAX || score->w_balanced > BS_SCORE_WEIGHT_MAX) {
    c->last_error = "bs_seq_run_scored_nominated_sampled: a weight is above BS_SCORE_WEIGHT_MAX";
    return BS_ERR_INVALID;
  }
  if (const int rc = seq_sample_refusals(c, stages, sample, "bs_seq_run_scored_nominated_sampled")) return rc;
  const SeqNomCall nc{priority, &own_row};
  return seq_run_impl(c, stages, out, &nc, score, sample);
}

int bs_seq_sample_read(bs_ctx* c, uint32_t p, uint32_t* start, uint32_t* visited, uint32_t* next_start) {
  if (!c) return BS_ERR_INVALID;
  if (!c->seq_sample_valid) { c->last_error = "bs_seq_sample_read: the context's last pass was not a successful sampled pass (bs_seq_run_scored_sampled or bs_seq_run_scored_nominated_sampled)"; return BS_ERR_STATE; }
  if (p != c->seq_score_p) { c->last_error = "bs_seq_sample_read: p is not the queue length of that pass"; return BS_ERR_INVALID; }
  if (const int rc = use_device(c)) return rc;
  const uint32_t* d = c->d_seq_sample.as<uint32_t>();
  const size_t nP = std::max<uint32_t>(p, 1);
  if (p && start) HIPCHK(c, hipMemcpy(start, d, (size_t)p * 4, hipMemcpyDeviceToHost));
  if (p && visited) HIPCHK(c, hipMemcpy(visited, d + nP, (size_t)p * 4, hipMemcpyDeviceToHost));
  if (next_start) HIPCHK(c, hipMemcpy(next_start, d + 2 * nP, 4, hipMemcpyDeviceToHost));
  return BS_OK;
}

int bs_seq_score_read(bs_ctx* c, uint32_t p, uint32_t* total, uint32_t* n_fit) {
  if (!c) return BS_ERR_INVALID;
  if (!c->seq_score_valid) { c->last_error = "bs_seq_score_read: the context's last pass was not a successful bs_seq_run_scored or bs_seq_run_scored_nominated"; return BS_ERR_STATE; }
  if (p != c->seq_score_p) { c->last_error = "bs_seq_score_read: p is not the queue length of that pass"; return BS_ERR_INVALID; }
  if (const int rc = use_device(c)) return rc;
  const uint32_t* d = c->d_seq_score.as<uint32_t>();
  const size_t nP = std::max<uint32_t>(p, 1);
  if (p && total) HIPCHK(c, hipMemcpy(total, d, (size_t)p * 4, hipMemcpyDeviceToHost));
  if (p && n_fit) HIPCHK(c, hipMemcpy(n_fit, d + nP, (size_t)p * 4, hipMemcpyDeviceToHost));
  return BS_OK;
}

int bs_seq_nominated_read(bs_ctx* c, uint32_t cap, uint32_t* id, uint32_t* pod, uint32_t* node, uint32_t* n_out) {
  if (!c || !n_out) return BS_ERR_INVALID;
  if (!c->seq_nom_valid) { c->last_error = "bs_seq_nominated_read: the context's last pass was not a successful bs_seq_run_nominated or bs_seq_run_scored_nominated"; return BS_ERR_STATE; }
  const uint32_t n = (uint32_t)c->seq_nom_id.size(), k = std::min(n, cap);
  if (k && (!id || !pod || !node)) { c->last_error = "bs_seq_nominated_read: an output array is NULL with rows to report"; return BS_ERR_INVALID; }
  if (k) {
    std::memcpy(id, c->seq_nom_id.data(), (size_t)k * 4);
    std::memcpy(pod, c->seq_nom_pod.data(), (size_t)k * 4);
    std::memcpy(node, c->seq_nom_node.data(), (size_t)k * 4);
  }
  *n_out = n;
  return BS_OK;
}

int bs_seq_run_nominated_flat(bs_ctx* c, uint32_t stages, uint32_t p, const int32_t* priority, const uint32_t* own_id, uint8_t* pf_code, uint32_t* pf_first_k,
                              int32_t* pf_leader, int32_t* pod_node, uint32_t cap, uint32_t* released_group, uint32_t* released_pods, int64_t* first_ns,
                              int64_t* ready_ns, int64_t* scalars_out, uint8_t* last_permitted) {
  bs_seq_out o{};
  o.last_permitted = last_permitted;
  o.pf_code = pf_code; o.pf_first_k = pf_first_k; o.pf_leader = pf_leader; o.pod_node = pod_node; o.cap = cap; o.released_group = released_group;
  o.released_pods = released_pods; o.first_ns = first_ns; o.ready_ns = ready_ns;
  const int rc = bs_seq_run_nominated(c, stages, p, priority, own_id, &o);
  if (scalars_out) {
    scalars_out[0] = o.n_released; scalars_out[1] = o.total_ns; scalars_out[2] = (int64_t)o.node_picks; scalars_out[3] = (int64_t)o.node_scans;
    scalars_out[4] = (int64_t)o.scan_rounds; scalars_out[5] = (int64_t)o.pick_rounds; scalars_out[6] = (int64_t)o.leader_folds;
    scalars_out[7] = (int64_t)o.table_builds;
  }
  return rc;
}

int bs_seq_run_scored_nominated_flat(bs_ctx* c, uint32_t stages, uint32_t p, const int32_t* priority, const uint32_t* own_id, uint32_t w_least, uint32_t w_most,
                                     uint32_t w_balanced, uint8_t* pf_code, uint32_t* pf_first_k, int32_t* pf_leader, int32_t* pod_node, uint32_t cap,
                                     uint32_t* released_group, uint32_t* released_pods, int64_t* first_ns, int64_t* ready_ns, int64_t* scalars_out,
                                     uint8_t* last_permitted) {
  bs_seq_out o{};
  o.last_permitted = last_permitted;
  o.pf_code = pf_code; o.pf_first_k = pf_first_k; o.pf_leader = pf_leader; o.pod_node = pod_node; o.cap = cap; o.released_group = released_group;
  o.released_pods = released_pods; o.first_ns = first_ns; o.ready_ns = ready_ns;
  const bs_seq_score score{w_least, w_most, w_balanced};
  const int rc = bs_seq_run_scored_nominated(c, stages, p, priority, own_id, &score, &o);
  if (scalars_out) {
    scalars_out[0] = o.n_released; scalars_out[1] = o.total_ns; scalars_out[2] = (int64_t)o.node_picks; scalars_out[3] = (int64_t)o.node_scans;
    scalars_out[4] = (int64_t)o.scan_rounds; scalars_out[5] = (int64_t)o.pick_rounds; scalars_out[6] = (int64_t)o.leader_folds;
    scalars_out[7] = (int64_t)o.table_builds;
  }
  return rc;
}

int bs_seq_run_scored_sampled_flat(bs_ctx* c, uint32_t stages, uint32_t w_least, uint32_t w_most, uint32_t w_balanced, uint32_t num_to_find, uint32_t start,
                                   uint8_t* pf_code, uint32_t* pf_first_k, int32_t* pf_leader, int32_t* pod_node, uint32_t cap, uint32_t* released_group,
                                   uint32_t* released_pods, int64_t* first_ns, int64_t* ready_ns, int64_t* scalars_out, uint8_t* last_permitted) {
  bs_seq_out o{};
  o.last_permitted = last_permitted;
  o.pf_code = pf_code; o.pf_first_k = pf_first_k; o.pf_leader = pf_leader; o.pod_node = pod_node; o.cap = cap; o.released_group = released_group;
  o.released_pods = released_pods; o.first_ns = first_ns; o.ready_ns = ready_ns;
  const bs_seq_score score{w_least, w_most, w_balanced};
  const bs_seq_sample sample{num_to_find, start};
  const int rc = bs_seq_run_scored_sampled(c, stages, &score, &sample, &o);
  if (scalars_out) {
    scalars_out[0] = o.n_released; scalars_out[1] = o.total_ns; scalars_out[2] = (int64_t)o.node_picks; scalars_out[3] = (int64_t)o.node_scans;
    scalars_out[4] = (int64_t)o.scan_rounds; scalars_out[5] = (int64_t)o.pick_rounds; scalars_out[6] = (int64_t)o.leader_folds;
    scalars_out[7] = (int64_t)o.table_builds;
  }
  return rc;
}

int bs_seq_run_scored_nominated_sampled_flat(bs_ctx* c, uint32_t stages, uint32_t p, const int32_t* priority, const uint32_t* own_id, uint32_t w_least,
                                             uint32_t w_most, uint32_t w_balanced, uint32_t num_to_find, uint32_t start, uint8_t* pf_code, uint32_t* pf_first_k,
                                             int32_t* pf_leader, int32_t* pod_node, uint32_t cap, uint32_t* released_group, uint32_t* released_pods,
                                             int64_t* first_ns, int64_t* ready_ns, int64_t* scalars_out, uint8_t* last_permitted) {
  bs_seq_out o{};
  o.last_permitted = last_permitted;
  o.pf_code = pf_code; o.pf_first_k = pf_first_k; o.pf_leader = pf_leader; o.pod_node = pod_node; o.cap = cap; o.released_group = released_group;
  o.released_pods = released_pods; o.first_ns = first_ns; o.ready_ns = ready_ns;
  const bs_seq_score score{w_least, w_most, w_balanced};
  const bs_seq_sample sample{num_to_find, start};
  const int rc = bs_seq_run_scored_nominated_sampled(c, stages, p, priority, own_id, &score, &sample, &o);
  if (scalars_out) {
    scalars_out[0] = o.n_released; scalars_out[1] = o.total_ns; scalars_out[2] = (int64_t)o.node_picks; scalars_out[3] = (int64_t)o.node_scans;
    scalars_out[4] = (int64_t)o.scan_rounds; scalars_out[5] = (int64_t)o.pick_rounds; scalars_out[6] = (int64_t)o.leader_folds;
    scalars_out[7] = (int64_t)o.table_builds;
  }
  return rc;
}

int bs_seq_run_scored_flat(bs_ctx* c, uint32_t stages, uint32_t w_least, uint32_t w_most, uint32_t w_balanced, uint8_t* pf_code, uint32_t* pf_first_k,
                           int32_t* pf_leader, int32_t* pod_node, uint32_t cap, uint32_t* released_group, uint32_t* released_pods, int64_t* first_ns,
                           int64_t* ready_ns, int64_t* scalars_out, uint8_t* last_permitted) {
  bs_seq_out o{};
  o.last_permitted = last_permitted;
  o.pf_code = pf_code; o.pf_first_k = pf_first_k; o.pf_leader = pf_leader; o.pod_node = pod_node; o.cap = cap; o.released_group = released_group;
  o.released_pods = released_pods; o.first_ns = first_ns; o.ready_ns = ready_ns;
  const bs_seq_score score{w_least, w_most, w_balanced};
  const int rc = bs_seq_run_scored(c, stages, &score, &o);
  if (scalars_out) {
    scalars_out[0] = o.n_released; scalars_out[1] = o.total_ns; scalars_out[2] = (int64_t)o.node_picks; scalars_out[3] = (int64_t)o.node_scans;
    scalars_out[4] = (int64_t)o.scan_rounds; scalars_out[5] = (int64_t)o.pick_rounds; scalars_out[6] = (int64_t)o.leader_folds;
    scalars_out[7] = (int64_t)o.table_builds;
  }
  return rc;
}

int bs_seq_run_flat(bs_ctx* c, uint32_t stages, uint8_t* pf_code, uint32_t* pf_first_k, int32_t* pf_leader, int32_t* pod_node, uint32_t cap,
                    uint32_t* released_group, uint32_t* released_pods, int64_t* first_ns, int64_t* ready_ns, int64_t* scalars_out,
                    uint8_t* last_permitted) {
  bs_seq_out o{};
  o.last_permitted = last_permitted;
  o.pf_code = pf_code; o.pf_first_k = pf_first_k; o.pf_leader = pf_leader; o.pod_node = pod_node; o.cap = cap; o.released_group = released_group;
  o.released_pods = released_pods; o.first_ns = first_ns; o.ready_ns = ready_ns;
  const int rc = bs_seq_run(c, stages, &o);
  if (scalars_out) {
    scalars_out[0] = o.n_released; scalars_out[1] = o.total_ns; scalars_out[2] = (int64_t)o.node_picks; scalars_out[3] = (int64_t)o.node_scans;
    scalars_out[4] = (int64_t)o.scan_rounds; scalars_out[5] = (int64_t)o.pick_rounds; scalars_out[6] = (int64_t)o.leader_folds;
    scalars_out[7] = (int64_t)o.table_builds;
  }
  return rc;
}
}  // extern "C"
