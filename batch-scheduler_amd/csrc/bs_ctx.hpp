// bs_ctx.hpp — the context behind the C ABI of include/bsched.h, and what the translation units that implement that ABI share: bsched.hip
// (contexts, loads, the batch) and the family units, every other tu_*.hip but tu_fast.hip (their entry points beside their kernels; what one
// family unit offers another is declared below, under the unit that defines it).
// Host code only: no kernel, and no header of a kernel family (the field types come from bs_kernels.hpp and the plain host headers).
#pragma once
#include <rccl/rccl.h>   // types and enums only: librccl itself is dlopen'ed on demand (hosts without RCCL can still load the library)

#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "bs_carve.hpp"
#include "bs_hostmem.hpp"
#include "bs_kernels.hpp"
#include "bs_lanes.hpp"
#include "bs_layouts.hpp"
#include "bs_pod_ranges.hpp"
#include "bs_preempt_clear_list.hpp"

namespace bs {

struct EventPair { hipEvent_t a, b; uint32_t id; };

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }   // LDS sizing and the two hand-added result blocks (ensure_hout, bs_batch_read)
// element n of a device array that may not exist yet (null + n is undefined behaviour even if nobody follows the pointer)
template <class T>
T* at(T* p, size_t n) { return p ? p + n : nullptr; }

// The eight columns of a group pack, for GroupsDev and GlPack
template <class D>
void group_cols(D& d, const GroupLayout& l, void* pk) {
  d.min_member = l.mm.in(pk); d.status_scheduled = l.sc.in(pk); d.matched = l.matched.in(pk); d.flags = l.flags.in(pk);
  d.cls = l.cls.in(pk); d.minres = l.minres.in(pk); d.mrpres = l.mrpres.in(pk); d.occupied = l.occ.in(pk);
}
// ... and beside the caller's arrays of a bs_groups_soa: f(piece, array) column by column, until one returns non-zero
template <class F>
int group_soa_cols(const GroupLayout& l, const bs_groups_soa& r, F f) {
  int rc;
  if ((rc = f(l.mm, r.min_member)) || (rc = f(l.sc, r.status_scheduled)) || (rc = f(l.matched, r.matched)) || (rc = f(l.flags, r.flags)) ||
      (rc = f(l.cls, r.cls)) || (rc = f(l.minres, r.min_resources)) || (rc = f(l.mrpres, r.min_resources_present)) || (rc = f(l.occ, r.occupied_by)))
    return rc;
  return 0;
}
// the rows of `r` into a pack laid out by `l` at `st` (host memory).  l.g > 0 rows: every piece holds exactly l.g of them
inline void stage_group_rows(const GroupLayout& l, void* st, const bs_groups_soa& r) {
  if (l.g) group_soa_cols(l, r, [st](auto piece, const auto* rows) { std::memcpy(piece.in(st), rows, piece.bytes()); return 0; });
}

// Defined in bsched.hip: the kernel groups' names (LAUNCHCHK) and the helpers that the family units call too.  Every entry point starts with
// use_device: a deferred group patch (bs_groups_apply) goes out now, unless the caller can take it along in its own launch (bs_pods_apply).
extern const char* const kKernelNames[BS_KERNEL_COUNT];
int use_device(bs_ctx* c, bool flush = true);
int settle_pending(bs_ctx* c);
int begin_reload(bs_ctx* c);   // use_device, settle_pending, steady_prev dropped: how bs_nodes_load, bs_fit_load / _build, bs_groups_load and bs_groups_list_apply open
NodesDev nodes_dev(const bs_ctx* c);
GroupsDev groups_dev(const bs_ctx* c);
PodsDev pods_dev(const bs_ctx* c);
uint32_t* pclass_dev(const bs_ctx* c);
void launch_nodes_assume(bs_ctx* c, const bs_node_request* records, uint32_t n);
void mirror_node_requests(bs_ctx* c, const bs_node_request* records, uint32_t n);
void rederive_nodes(bs_ctx* c, uint32_t base0 = 0, uint32_t m_before = 0);
int group_layout(bs_ctx* c, uint32_t G, bool headroom);
int group_counts(bs_ctx* c);
int analyse_groups(bs_ctx* c, bool rearm_scratch = true, const bs_group_delta* deltas = nullptr, uint32_t ndeltas = 0, bool defer = false);
int maybe_analyse_epochs(bs_ctx* c);
int check_handover(bs_ctx* c);
// Defined in tu_wait.hip: the wait table's removal core in its release form (the rows of the listed groups leave by the stable compaction,
// nothing else is touched), with the rows' groups as a third column: bs_groups_list_apply drops the rows of removed groups through it.
int wait_release_rows(bs_ctx* c, const char* who, uint32_t count, const uint32_t* group, uint32_t cap, uint32_t* id_out, uint32_t* node_out, int32_t* group_out,
                      uint32_t* n_out);
int32_t* wait_group_column(const bs_ctx* c);   // the live table's group column ([wait_w] rows)
// Defined in tu_wait.hip: the wait core's launch sequence in its by-id release form (mode by id, no node side, no forget, no expire), cut
// where bs_bound_bind puts its own kernels: wait_bind_front launches k_wt_mark -> k_wt_scan1 -> k_wt_scan2 over the listed ids (and k_wt_walk
// when `walk`: the pass's chains as wnode[P]) and names what those left on the device; wait_bind_back launches k_wt_move<S> -> k_wt_finish
// (the twin and this call's scratch only; the marks come off on every path).  Nothing waits for the stream.  After the caller's one wait:
// wait_bind_waited (the marks are clean again), wait_bind_verdict over the info words it read back (BS_OK, or the refusal with last_error
// set), and on success wait_bind_commit (the twin becomes the table).
struct WaitBind {
  const uint32_t *id = nullptr, *node = nullptr, *pres = nullptr;   // the live table's columns, W rows
  const int32_t* group = nullptr;
  const int64_t* req = nullptr;                                     // [L][stride]
  uint32_t stride = 1, W = 0;
  const uint32_t* mark = nullptr;                                   // [mark_n] list position + 1 of a listed id
  uint32_t mark_n = 0;
  uint32_t* info = nullptr;                                         // the core's four info words
  const uint32_t* err = nullptr;                                    // the error word among them
  const int32_t* wnode = nullptr;                                   // [P] the node of a pod that waits in the pass's chains, else -1 (walk only)
  uint32_t n_wait = 0;
  std::vector<uint8_t> core;                                        // the core's own device struct of this call
};
int wait_bind_state(bs_ctx* c, const char* who);   // BS_OK, or why the wait table cannot be used now (bs_wait_release's test)
int wait_bind_front(bs_ctx* c, const char* who, uint32_t n_wait, const uint32_t* wait_id, bool walk, WaitBind& wb);
int wait_bind_back(bs_ctx* c, const WaitBind& wb);
void wait_bind_waited(bs_ctx* c, const WaitBind& wb);
int wait_bind_verdict(bs_ctx* c, const char* who, const WaitBind& wb, const uint32_t info[4]);
void wait_bind_commit(bs_ctx* c, const WaitBind& wb, const uint32_t info[4]);
// Defined in tu_bound.hip: the back half of every patch of the bound table, for a delta block that is on the device already.  `a` names the
// delta (remove ids, the inserts sorted by (node, importance)) and the scratch in d_pre; the call sizes the second allocation for
// b - n_remove + n_insert entries, points `a` at the live table, launches k_ba_scatter .. k_ba_merge, waits once, judges the error word
// and swaps the allocations (table, entry count, id space + n_insert, the group maximum).  hooks (NULL: none): before_wait enqueues the
// caller's own launches and copies behind the merge; verdict runs after the wait and before the error word is judged: the caller's own
// error words (non-zero: returned, nothing is swapped) and the group maximum where only the device knows it.
struct BoundApplyDev;
struct BoundBlockHooks {
  std::function<int()> before_wait;
  std::function<int(uint32_t ba_err, int32_t& gmax)> verdict;
};
int bound_apply_block(bs_ctx* c, const char* who, BoundApplyDev& a, int32_t gmax, const BoundBlockHooks* hooks = nullptr);
int32_t* bound_group_column(const bs_ctx* c);   // the live table's group column ([bound_b] entries)
// Defined in tu_bound.hip: how the table's two allocations trade places, for every call that rewrites the table (the patch above, the plans'
// compaction in tu_preempt.hip, bs_bound_nodes_apply).  bound_twin lays the second allocation out for b entries on n nodes (`lay`) and makes
// room for them: exactly, or with a quarter of headroom whenever it has to grow; with `nw`, that struct names the second allocation's columns
// as a compaction target.  bound_swap, after the wait: the second allocation becomes the table (pointer, capacity, layout, entry count).
struct CompactDev;
hipError_t bound_twin(bs_ctx* c, uint32_t n, uint32_t b, bool headroom, BoundLayout& lay, CompactDev* nw = nullptr);
void bound_swap(bs_ctx* c, const BoundLayout& lay, uint32_t b);
// Defined in tu_nominated.hip: what the preemption calls use the nominated-pod table through.  nom_view: what the victim search reads (null
// without a table or without rows); nom_state: BS_OK, or why the table cannot be patched now; nom_preempt_state: BS_OK, or the refusal of
// rows made for another node count; nom_refusal: a check code of bs_nominated_check.hpp as last_error and status; nom_apply_rows:
// bs_nominated_apply behind its checks (BS_PREEMPT_NOMINATE's append; BS_PREEMPT_CLEAR_LOWER's removals ride the same rewrite);
// nom_clear_list: k_nc_list on the context's stream behind a BS_PREEMPT_CLEAR_LOWER resolve — thr / first are that resolve's working
// state ([n], bs_preempt_clear.hpp), sorig its slot-to-caller column; the live table's rows below their node's threshold go to cols
// ([4][max(rows, 1)]: id, node, priority, by) compacted in ascending id, their number to *count.  Launch only: the caller waits.
struct NomView;
const NomView* nom_view(const bs_ctx* c);
int nom_state(bs_ctx* c, const char* who);
int nom_preempt_state(bs_ctx* c, const char* who);
int nom_refusal(bs_ctx* c, const char* who, int bad);
int nom_apply_rows(bs_ctx* c, uint32_t R, const uint32_t* remove_id, uint32_t I, const uint32_t* pod_index, const uint32_t* node, const int32_t* priority);
void nom_clear_list(bs_ctx* c, const uint32_t* thr, const uint32_t* first, const uint32_t* sorig, uint32_t* cols, uint32_t* count);
// ... and what the sequential pass under rule S (bs_seq_run_nominated, tu_seq.hip) uses it through, beside nom_state and nom_view.  The pass
// keeps the consumed bytes in its own scratch (zeroed before its launch) and translates ids to rows by nom_live, which is the table's order.
// nom_drop_flagged: the rows whose byte in the DEVICE array flag[rows] is set leave by the stable compaction into the twin (k_nm_move<S> ->
// k_nm_chains, bs_nominated_apply's tail), the twin becomes the table and nom_live loses `gone`, the same rows' ids, ascending.  One wait.
int nom_drop_flagged(bs_ctx* c, const uint8_t* flag, const std::vector<uint32_t>& gone);

}  // namespace bs

using namespace bs;   // bs_ctx is the C ABI's struct, at global scope, and names a bs:: type on nearly every line; so do the entry points of every unit

struct bs_ctx {
  bs_config cfg{};
  uint32_t L = 4, S = 0, LP = 4;
  std::string last_error;

  // ---- nodes
  bool have_nodes = false, have_fit = false, have_groups = false, have_pods = false;
  uint32_t N = 0, Ncap = 0, M = 0, C = 0, fit_words = 0;
  DevBuf d_alloc, d_nreq, d_apres, d_rpres, d_nflags, d_fit, d_kmap, d_m, d_left4, d_lglob;
  DevBuf d_fitarena, d_fitcols;                  // bs_fit_build inputs / label columns
  std::vector<int64_t> h_alloc, h_nreq;          // [L][N] mirrors (churn + read-back)
  std::vector<uint32_t> h_apres, h_rpres, h_kmap;
  std::vector<uint8_t> h_nflags;
  std::vector<uint32_t> h_fit;                   // [C][fit_words]

  // ---- groups
  uint32_t G = 0, n_uncaptured = 0;   // groups without a pod (first-pod capture possible)
  std::vector<uint32_t> h_gmatched, h_gcls;
  std::vector<uint8_t> h_gflags;
  int32_t steady_table = -1;        // the one table every reservation query uses when no capture can occur, -1 unknown
  // Speculation (bs_batch_run): a group patch re-runs findMaxPG on the device, and the host would have to wait for its answer (the
  // table id) before it can launch the chain — ~4 us of idle GPU and ~10 us of spinning per cycle.  In a steady state the answer is
  // nearly always the one of the cycle before, so the chain is launched on THAT and checked when the results are first asked for
  // (batch_settle): a wrong guess costs one re-run, a right one nothing.
  int32_t steady_prev = -1;          // steady_table of the last resolved analysis
  bool spec_active = false;          // the last batch ran on a guessed table that nobody has checked yet
  int32_t spec_table = -1;
  uint32_t spec_stages = 0;
  uint32_t no_spec = 0;              // BS_NO_SPECULATE=1
  uint64_t n_spec = 0, n_spec_miss = 0;
  // BS_HOST_PROBE=1: where bs_batch_run's host time goes (ns, accumulated; printed at bs_destroy)
  uint32_t host_probe = 0;
  uint64_t hp_ns[6] = {0, 0, 0, 0, 0, 0}, hp_n = 0, hp_t0 = 0, hp_t1 = 0;
  uint64_t early_filter_min = 200000000ull;   // pod x node pairs from which Filter overlaps the scan
  // groups live in ONE device allocation (one pinned-staged H2D per load); d_info / h_info carry what findMaxPG
  // found for the loaded state back to the host without a stream wait (see resolve_groups)
  DevBuf d_gpack, d_info, d_gdelta;
  DevBuf d_gpack2, d_glist;          // bs_groups_list_apply: the allocation the new group pack is gathered into (swapped with d_gpack); its per-call scratch
  GroupLayout glay;                  // the live pack's layout (group_layout)
  int32_t info_tag = 0, kinfo_tag = 0;
  bool info_pending = false, kinfo_pending = false;
  uint32_t max_group_cls = 0, max_pod_cls = 0;   // largest fit class any HAS_POD group / grouped pod names (checked against C per batch)
  uint32_t h_K = 0;                  // request classes of the loaded pods (valid after resolve_pods)
  uint32_t k_bound = 0;              // while kinfo_pending: an upper bound of the class count the device holds (last known K + pods inserted since)

  // ---- pods
  uint32_t P = 0;
  // pods live in ONE device allocation (one H2D per batch from a pinned staging buffer); outputs likewise (one D2H)
  DevBuf d_pack[2], d_outpack;       // two pod packs: bs_pods_apply compacts from the current one into the other
  PodLayout lay[2], stage_lay;       // their layouts, and the staging buffer's own
  uint32_t cur_pack = 0;
  bool last_use_classes = false;
  uint32_t map_p = 0;                // pods the staging buffer is currently mapped for (bs_pods_map), 0 = not mapped
  // queue-resident cycle (bs_pods_apply, bs_queue.hpp)
  DevBuf d_gstat2, d_cdir, d_pdir, d_ckeys, d_cpres, d_pkeys;
  uint32_t gstat_cur = 0;            // which of d_gstat / d_gstat2 holds the per-group minima of the resident queue
  uint32_t pair_cap = 0, dir_slots = 0;   // id space of classes / pairs between two derivations; hash slots of each directory
  uint32_t ids_used = 0;             // upper bound of the class / pair ids drawn since the last derivation
  bool rep_valid = false;            // d_cls_rep / d_cls_id / pair ids still name pods of the resident queue (no compaction since)
  bool dirs_ready = false;           // the directories match the resident queue's classes and pairs
  uint32_t id_room = 0;              // BS_ID_ROOM: ids beyond the queue length (0 = the default: as many again + 1024)
  uint32_t serial_insert_max = 2048; // more inserted pods than this: re-derive in parallel instead of the insert wave
  uint64_t n_applies = 0, n_rederives = 0;
  OutLayout olay;                    // the result pack's layout (layout_out), shared by d_outpack, h_hout and h_rstage

  // ---- batch scratch / outputs
  DevBuf d_first_elig, d_first_owner, d_first_reject, d_first_pod, d_cap_epoch;
  DevBuf d_epoch, d_nepochs, d_leader_epoch, d_panic_epoch;
  DevBuf d_tcode, d_stage, d_leader_raw, d_first_row, d_first_row64, d_scan_rec, d_feas_rec, d_chunk_rec, d_qreq_s, d_qflags_s, d_qpos;
  DevBuf d_needed, d_qcount, d_ticket, d_desc;
  bool scratch_armed = false;
  bool side_ready = false;      // desc[] of the steady-state table is in place for the next batch   // per-group minima are INF (k_init ran, or the previous batch's k_tally re-armed them)
  DevBuf d_tables, d_kp, d_stats, d_fparams, d_fflags, d_chunk_tot, d_blk_scratch, d_gmax, d_chunk_kp;
  // request slots (see BatchDev): classes of the loaded pods + per-batch slot arrays
  DevBuf d_cls_slots, d_cls_rep, d_cls_id, d_qtab_s, d_fu_slot, d_uparams, d_uflags, d_uclaim, d_fu_bitmap, d_fu_feas;
  DevBuf d_nodew;                    // node words of the batch (BatchDev::nodew): 3 tables x (W + 2) word pairs + the two leaders' maxSingle
  bool batch_void = false;           // the last batch's results must not be handed out (check_handover); cleared by the next bs_batch_run
  uint32_t tp_tmin = 768;            // BS_TP_TMIN: tiles of Filter slots from which the transposed items take pairs of tiles (x ranks on a sharded context)
  bool no_nodew = false;             // BS_NO_NODEW=1: the transposed Filter item derives the node-only masks of every block itself (rounds 4-5; A/B switch)
  uint32_t slot_keep = 0xFFFFFFFFu;   // BS_HASH_SLOT_BITS (tests): directory probes start at hash & slot_keep
  uint32_t cls_cap = 0, hash_keep = 0x7FFFFFFFu, n_nominres = 0, scan_slots_cap = 0, filter_slots_cap = 0;
  DevBuf d_fl_bitmap, d_admit, d_ready, d_gcount, d_admit64, d_own_start;
  bool owner_ready = false;          // own_start[] matches the resident queue and the group count (sharded contexts only)
  // fast path (bs_fast.hpp)
  DevBuf d_order_rank, d_sort;         // queue ordering: per-group order ranks; inputs | index ping-pong | permutation
  uint32_t order_g = 0;
  DevBuf d_gstat, d_pair_next, d_pair_firstq, d_first_reach, d_qstamp_s, d_fast_reject, d_epoch_group;
  bool pairs_ready = false;          // d_gstat / pairs match the loaded pods and G
  bool bitmap_valid = false;         // d_fl_bitmap holds the expanded rows of the last batch
  bool last_fast = false;
  bool batch_since_pods = false;     // a batch ran over the loaded pods (its slot mode is the one the rows have)
  size_t off_hfeas = 0, off_htag = 0; // in h_hout
  uint32_t hstride = 0;
  int32_t host_tag = 0;
  bool last_host_out = false;
  uint32_t no_fast = 0;
  // positional three-launch chain (bs_epoch.hpp): analysis of (groups, pods) kept across batches
  DevBuf d_run_of_epoch, d_run_leader, d_gslot, d_gfirstq;
  bool epochs_ready = false, einfo_pending = false;
  int32_t einfo_tag = 0;
  uint32_t h_R = 0, h_eflags = 0, no_epoch = 0;
  uint32_t last_chain = 0;           // 0 general chain, 1 steady-state chain, 2 positional chain
  uint32_t last_rows = 0;            // Filter slot rows of the last positional batch
  // single-query scratch
  DevBuf d_sq;
  DevBuf d_seq;                      // bs_seq_run: scaled allocatables, keys, per-gang / per-pod bookkeeping, results
  // bs_seq_expire / bs_seq_waiting_read: the waiting state the last pass left in d_seq (chains, heads, counts) is valid from a successful
  // bs_seq_run until the first call that renumbers what it indexes (queue loads / patches, node loads / APPEND / REMOVE, group loads)
  bool seq_wait_valid = false;
  Piece<unsigned long long> seq_o_wait;
  Piece<uint32_t> seq_o_head, seq_o_nwait;
  Piece<int32_t> seq_o_node;         // the pass's pod_node block (bs_bound_bind reads a placed pod's node there)
  // bs_seq_nominated_read: the rows the last pass consumed (ascending id), valid while the last pass was a successful bs_seq_run_nominated
  bool seq_nom_valid = false;
  std::vector<uint32_t> seq_nom_id, seq_nom_pod, seq_nom_node;
  // bs_seq_score_read: total[P] | n_fit[P] of the last pass, valid while that pass was a successful bs_seq_run_scored over seq_score_p pods
  DevBuf d_seq_score;
  bool seq_score_valid = false;
  uint32_t seq_score_p = 0;
  // bs_seq_sample_read: start[P] | visited[P] | next_start of the last pass, valid while that pass was a successful sampled one (rule F) over
  // seq_score_p pods; every other pass clears the flag
  DevBuf d_seq_sample;
  bool seq_sample_valid = false;
  DevBuf d_sexp;                     // per-call scratch: block totals, slots, rows, dirty list, records
  DevBuf d_sexp_nodes;               // per-node delta [L][N], key bits, dirty words: zero between calls (k_se_nodes re-zeroes what it read)
  uint32_t sexp_n = 0, sexp_l = 0;   // the layout d_sexp_nodes was zeroed for
  bool sexp_clean = false;
  // the resident Permit-wait table (bs_wait_*, bs_wait.hpp): waiting pods that outlive their pass.  Two allocations of the same layout: the
  // live one (wait_cur) and the twin a compaction writes into and a growing park copies into; they swap on success.  Valid while the node
  // count and the group count are the ones it was created for.
  bool have_wait = false;
  uint32_t wait_w = 0, wait_ids = 0;   // rows; the id space: rows at the last bs_wait_load plus what bs_wait_park added since
  uint32_t wait_n = 0, wait_g = 0;     // node count and group count at the load
  DevBuf d_wait[2];
  uint32_t wait_cap[2] = {0, 0};       // rows each allocation is laid out for (the req lane stride)
  uint32_t wait_cur = 0;
  DevBuf d_wait_scr;                   // per-call scratch: block totals, positions, rows, per-list results, dirty list, records
  DevBuf d_wait_nodes;                 // per-node delta [L][N], key bits, dirty words: zero between calls (k_wt_nodes re-zeroes what it read)
  DevBuf d_wait_gmark, d_wait_imark;   // marks by group [G] / by id [id space]: zero between calls (k_wt_finish takes them off)
  bool wait_nodes_clean = false, wait_gmark_clean = false, wait_imark_clean = false;
  uint32_t table_slots = 0, table_mcap = 0;

  uint32_t rank = 0, nranks = 1;
  bool reduce_external = false;      // partitioned mode: tally only, the caller reduces and calls bs_batch_finish
  uint32_t* ext_admit = nullptr;     // caller-owned device memory for the admit counters
  int32_t sop_leader0 = -1;
  uint32_t last_stages = 0;
  // Batch counters.  batch_seq: monotonic, 64 bit (timing sampling, statistics).  stamp_ctr in [0, 65534]: slot stamps are
  // 1 + stamp_ctr (16 bits in the slot words); when it comes round to 0 the stamped arrays are zeroed, so a slot nobody wrote
  // for 65535 batches cannot look live again.  key_seq in [1, 0xFFFFFFFE]: the 64-bit atomicMin keys carry ~key_seq in the
  // high word ("a newer batch always wins", never all-ones = the 'none' the arrays are born with); when it runs out it
  // restarts at 1 behind a re-fill of the keyed arrays with 'none' (once per 2^32 - 2 batches).
  uint64_t batch_seq = 0;
  uint32_t stamp_ctr = 1, key_seq = 1;
  bool rekey_pending = false;
  bool batch_pending_finish = false;
  bool groups_launch_pending = false; // bs_groups_apply left its (inline) deltas + findMaxPG for the next launch: k_pods_apply takes them along, anything else flushes
  DeltaPack pending_dp{};
  uint32_t no_fuse_final = 0;        // BS_NO_FUSE_FINAL: launches B and C always as separate launches
  uint32_t tp_filter = 6;            // BS_TP_FILTER (throughput regime = more than 16 tiles of class slots): 0 = scan and Filter roles in one launch (k_fast_scan_filter: rounds 2-4),
                                     // 1..4 = k_fast_scan, then k_fast_filter<4,DB> / <2,DB> / <2,!DB> / k_fast_filter_w7 (109 / 93 / 75 / 72 VGPRs),
                                     // 5 = k_fast_scan, then k_fast_filter_t (the transposed item, bs_filter_t.hpp: 64 VGPRs),
                                     // 6 / 7 = one launch, Filter role by the transposed item (7: the Filter blocks first),
                                     // 8 = as 5, the two launches side by side on two streams
  uint32_t tp_share = 0;             // BS_TP_SHARE: scan shares per tile of class slots when launch B is not the fused form (at most);
                                     // 0 = 2 in the throughput regime, 64 otherwise (what the sweeps of profiles/r04c_* say)
  uint32_t tp_fwaves = 0;            // BS_TP_FWAVES: waves the Filter work of that regime is cut for; 0 = 16384 from 65 536 (tile, two node
                                     // blocks) units on, filter_waves below; an explicit BS_FILTER_WAVES rules
  bool filter_waves_env = false;
  uint32_t tp_split = 0;             // BS_TP_SPLIT: the transposed Filter items are cut for tp_split x the launched waves and dealt out tile quad by
                                     // tile quad (filter_loop_t, by_tile); 0 = 2 on a rank of a sharded context (bs_shard_set), 1 otherwise.
                                     // Class ids follow the queue (k_pod_class_ids), so all but 1 / nranks of the slot tiles are idle on a rank and
                                     // return at their first load; the live ones are cut finer so that they spread over more of the launched
                                     // waves.  cfg4 all-distinct, rank 0 of 8 (profiles/r05_shard_scaling.md): 60 us at x2, 63 at x4, 74 at x8
                                     // (an item's prologue — requests, bounds, first node block — is ~4 us whatever its length).
  int fused_blocks_resident = -1;    // whole-chip residency of k_fast_scan_filter_final (blocks), -1 = not asked yet
  int step_a_resident[2] = {-1, -1};          // ... of k_fast_step_a
  // The one-launch form of launch A + the scan / Filter roles (k_fast_step_a, then k_fast_final), where it applies (the latency regime: at most 256
  // classes, 64 table chunks, 4 scalar lanes; the second batch over a queue onwards).  BS_STEP_A=3, the DEFAULT: the whole-step form — the class-slot
  // form below whose pod blocks go on to the final verdicts inside the same launch (one launch per step; form 2 where it does not apply).  Which form a step takes, its grid and its ticket advances:
  // step_a_plan (bs_step_geom.hpp).
  // BS_STEP_A=2: the class-slot form — class_slots_block publishes every class's slots from the class directory, the pod blocks gate nobody; k_fast_final
  // follows as a second launch.  BS_STEP_A=1: every pod block publishes (kept as a tested experiment).  BS_STEP_A=0: off.  Step times: BASELINE.md.
  uint32_t step_a_form = 3;
  bool step_a_on = true;
  uint32_t step_shares = 8;          // BS_STEP_SHARES: blocks that share one table chunk's class slots (at most; step_a_plan's nshares, bs_step_geom.hpp).  8 was the fastest of 2 / 4 / 8 / 16 under BS_STEP_A=2
                                     // (profiles/r06_step_a_class_slots_shares.txt); the whole-step form has not been swept
  uint32_t test_timeout_after = 0;   // BS_TEST_HANDOVER_TIMEOUT=n (test hook): the n-th one-launch step reports a timed-out hand-over as the device would
  uint32_t test_pc_chunk_nodes = 0;  // BS_TEST_PC_CHUNK_NODES=n (test hook): nodes per chunk of the preemption grids (bs_preempt_geom.hpp); 0 = the shipped geometry
  uint32_t tk_pods = 0, tk_tab = 0;  // values of ticket[8] / ticket[9] the next k_fast_step_a starts from (never reset: wrap-safe differences)
  uint32_t tk_p1 = 0, tk_done = 0;   // ... of the spread counter at kTkP1 (form 3: the pod blocks' first halves); tk_done: of the counter at kTkDone (large queues: every table / Filter block adds once)
  // form 3's gang-aligned pod ranges (bs_pod_ranges.hpp): computed by bs_pods_load, dropped by bs_pods_apply (256 pods per block until the next load)
  bool pod_ranges_on = true;         // BS_POD_RANGES=0: 256 pods per block always (A/B switch)
  bool ranges_valid = false;         // (also dropped by a bs_groups_load that changes the group count: the local flags are per group)
  uint32_t nranges = 0;
  PodRanges h_ranges;
  std::vector<uint32_t> h_pod_ranges;  // BatchDev::pod_ranges as uploaded (the copy reads it: rewritten only after h_stage.wait)
  DevBuf d_pod_ranges;
  bool last_step_a = false;
  uint32_t scan_share_override = 0, no_fuse_filter = 0, early_forced = 0, target_waves = 8192, filter_waves = 8192, collect_stats = 0;
  uint32_t general_waves = 4096;     // scan grid cap of the general chain (tools/cold_sweep.py)
  bs_batch_stats stats{};

  // ---- timing
  std::vector<EventPair> events;
  size_t events_used = 0;
  bs_timing timing{};

  // ---- native RCCL (dlopen'ed on demand; entry points resolved once in bs_comm_init)
  void* rccl_handle = nullptr;
  void* comm = nullptr;
  decltype(&ncclAllReduce) rccl_allreduce = nullptr;
  decltype(&ncclCommDestroy) rccl_destroy = nullptr;
  uint32_t launches = 0;             // kernel launches of the last batch
  // BS_BATCH_FILTER_DENY (bs_fdeny.hpp)
  DevBuf d_fd_event, d_fd_in, d_fd_flag;
  bool fd_on = false;                // the run being launched replays Filter's deny entry
  bool fd_active = false;            // the last batch did, and nobody has looked at its flag words yet (fd_settle)
  uint32_t first_reach_hint = 0xFFFFFFFFu;   // bs_first_reach_hint (partitioned mode), reset by every queue load / patch
  bool fd_unsynced = false;          // a BS_BATCH_FILTER_DENY batch was launched and the stream has not been waited for since
  bool fd_in_live = false;           // a fixed-point re-run: the chains honour d_fd_in
  uint32_t fd_iter = 0, fd_stages = 0, fd_seq_inv = 0;
  uint64_t n_fd_reruns = 0;          // fixed-point re-runs so far (bs_batch_stats_get)
  // preemption (bs_preempt.hpp): the bound-pod table, CSR by node in importance order, in one allocation; per-call scratch
  bool have_bound = false;
  uint32_t bound_b = 0, bound_n = 0;  // entries, node count at the load
  int32_t bound_max_group = -1;      // largest group index the table names (checked against the group count per call)
  DevBuf d_bound, d_pre;
  DevBuf d_bound2;                   // bs_preempt_commit's compaction target (swapped with d_bound)
  BoundLayout blay{};
  uint32_t bound_ids = 0;            // the id space of bs_bound_pdb_set: entries at the last bs_bound_load plus what bs_bound_apply inserted since
  std::vector<uint32_t> pre_npv;     // PDB-violating victims per preemptor of the last preemption call (bs_preempt_pdb_read)
  bool have_pre_npv = false;
  // bs_preempt_gang_read: slot_voided[count] / group_placed[g] of the last bs_preempt_commit_gang, while it is the last preemption call
  std::vector<uint8_t> gang_voided;
  std::vector<uint32_t> gang_placed;
  bool have_gang = false;
  // resident PodDisruptionBudgets (bs_pdb.hpp): allowed[pdb_n], and the PDBs of every covered bound-pod id as a CSR by id; dropped by bs_bound_load
  bool have_pdb = false;
  uint32_t pdb_n = 0, pdb_covered = 0, pdb_members = 0;   // PDBs, ids the CSR covers, membership entries (= moff[pdb_covered])
  DevBuf d_pdb_allowed, d_pdb_moff, d_pdb_member;
  // the resident nominated-pod table (bs_nominated_*, bs_nominated.hpp).  Two allocations of one layout, as the wait table: the live one
  // (nom_cur) and the twin every bs_nominated_apply writes into; they swap on success.  Valid while the node count is the one it was made for.
  bool have_nom = false;
  uint32_t nom_w = 0, nom_ids = 0;     // rows; the id space: rows at the last bs_nominated_load plus what was inserted since
  uint32_t nom_n = 0;                  // node count at the load
  DevBuf d_nom[2];
  uint32_t nom_cap[2] = {0, 0};        // rows each allocation is laid out for (the req lane stride, nnext's length)
  uint32_t nom_ncap[2] = {0, 0};       // ... and nodes (nhead's length)
  uint32_t nom_cur = 0;
  std::vector<uint32_t> nom_live;      // the table's ids, ascending: what bs_nominated_apply checks its remove list against before any launch
  std::vector<uint32_t> pre_nom;       // row id per preemptor of the last BS_PREEMPT_NOMINATE call (bs_preempt_nominated_read)
  bool have_pre_nom = false;
  ClearedRows pre_clr;                 // the rows the last BS_PREEMPT_CLEAR_LOWER call cleared (bs_preempt_cleared_read; bs_preempt_clear_list.hpp)

  // ---- streams, events, pinned host memory.  Declared LAST and in this order: members are destroyed in reverse, so the pinned buffers
  // and events go first, then stream3, then stream, and only then the DevBufs above (bs_destroy has waited for both streams).
  Stream stream;
  Stream stream3;                    // early Filter: runs beside the node scan when no capture can occur
  Event ev_query, ev_filter;
  PinnedBuf<int32_t> h_info{PinWait::None, hipHostMallocMapped | hipHostMallocCoherent};   // [16], kernels write it directly; its words by name: enum HInfo (bs_kernels.hpp, the device stores use it too)
  PinnedBuf<> h_gstage{PinWait::Event};   // groups pack, then deltas
  PinnedBuf<> h_glstage{PinWait::Stream}; // bs_groups_list_apply's delta (its rows as a group pack, the remove and update lists), read in place by k_gl_gather
  PinnedBuf<> h_stage{PinWait::Event};    // pod staging; busy until the last H2D out of it is through (bs_pods_load does not wait for it)
  PinnedBuf<> h_dstage{PinWait::Stream};  // the delta the apply kernel reads in place (no event per apply: bs_pods_apply)
  PinnedBuf<> h_nstage{PinWait::Event};   // node requests of bs_nodes_assume
  PinnedBuf<> h_pdbstage{PinWait::Stream};  // bs_pdb_allowed_apply's (index, value) pairs, read in place by k_pdb_allowed
  // result staging (bs_batch_read) and, in latency mode, the pinned result pack the last launch writes itself
  PinnedBuf<> h_rstage;
  PinnedBuf<> h_hout{PinWait::None, hipHostMallocMapped | hipHostMallocCoherent};            // [outpack layout | feas[hstride] | tag]
  PinnedBuf<uint64_t> h_hrows{PinWait::None, hipHostMallocMapped | hipHostMallocCoherent};   // [W + 1][hstride]
};

// h_info's words by name (volatile: a kernel may be writing them); hinfo_at: the word's address for a kernel (nullptr before the block exists)
inline int32_t hinfo_get(const bs_ctx* c, HInfo w) { return static_cast<volatile const int32_t*>(c->h_info.p)[w]; }
inline void hinfo_set(bs_ctx* c, HInfo w, int32_t v) { static_cast<volatile int32_t*>(c->h_info.p)[w] = v; }
inline int32_t* hinfo_at(const bs_ctx* c, HInfo w) { return c->h_info.p ? c->h_info.p + w : nullptr; }

#define HIPCHK(ctx, call)                                                                         \
  do {                                                                                            \
    hipError_t _e = (call);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(_e);                      \
      return BS_ERR_HIP;                                                                          \
    }                                                                                             \
  } while (0)
// a failed launch is reported with the kernel group it belongs to (bs_kernel_name)
#define LAUNCHCHK(ctx, id)                                                                         \
  do {                                                                                             \
    hipError_t _e = hipGetLastError();                                                             \
    if (_e != hipSuccess) {                                                                        \
      (ctx)->last_error = std::string("launch of kernel group '") + kKernelNames[id] + "': " + hipGetErrorString(_e); \
      return BS_ERR_HIP;                                                                           \
    }                                                                                              \
  } while (0)
