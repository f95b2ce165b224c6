// bs_launch.hpp — the launch wrappers that live in translation units of their own (tu_fast.hip, tu_seq.hip), so that the library builds
// in parallel and a change to one kernel family recompiles that family only.  Kernels in the shared headers are `inline __global__`:
// each translation unit emits exactly the kernels it launches.
// A wrapper picks the instantiation for the context's scalar-lane count by one of the three rules of bs_lanes.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_kernels.hpp"
#include "bs_lanes.hpp"

namespace bs {

inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// what the wrappers of the steady-state chain's second launch need from the context
struct FastLaunch {
  hipStream_t stream;
  uint32_t S, M, P, filter_waves, filter_slots_cap, tp_filter;
  int device;
  uint32_t filter_split = 0;   // waves the transposed Filter items are CUT for (0 = filter_waves, the grid): a rank of a sharded job cuts finer, see run_fast
};
void launch_fast_bc(const FastLaunch& c, dim3 grid, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const BatchDev& b, const BatchDev& bt,
                    const BatchParams& prm, uint32_t nseg, uint32_t scan_blocks, uint32_t filter_blocks);
void launch_fast_b(const FastLaunch& c, dim3 grid, const PodsDev& pd, const NodesDev& nd, const BatchDev& bt, const BatchParams& prm, uint32_t nseg,
                   uint32_t scan_blocks);
void launch_fast_scan(const FastLaunch& c, dim3 grid, const BatchDev& bt, const BatchParams& prm, uint32_t nseg);
void launch_fast_bt(const FastLaunch& c, dim3 grid, const NodesDev& nd, const BatchDev& bt, const BatchParams& prm, uint32_t nseg, uint32_t scan_blocks);
void launch_fast_filter(const FastLaunch& c, dim3 grid, const PodsDev& pd, const NodesDev& nd, const BatchDev& bt, const BatchParams& prm);
int fused_residency_query(const FastLaunch& c);
// round 5: launch A + the scan / Filter roles in one launch (k_fast_step_a<S>, S <= 4 or the generic-lane instantiation)
void launch_fast_step_a(const FastLaunch& c, dim3 grid, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const BatchDev& b, const BatchDev& bt,
                        const BatchParams& prm, const TableDesc* forced, uint32_t nchunks, uint32_t query_blocks, uint32_t nshares, uint32_t filter_blocks,
                        uint32_t tk_pods0, uint32_t tk_tab0, uint32_t param_blocks, const int64_t* ckeys, const uint32_t* cpres, uint32_t kcap,
                        uint32_t whole, uint32_t tk_p1, uint32_t tk_done, uint32_t forced_cls);
int step_a_residency_query(const FastLaunch& c, bool whole);      // blocks of k_fast_scan_filter_final<S> the chip holds at once (0 = unknown)

struct SeqDev;
struct SeqParams;
void launch_seq(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq, const SeqParams& prm);

// the Permit timeout (tu_seq_expire.hip, bs_seq_expire.hpp): k_se_scan1 + k_se_scan2 (counts, row offsets, the kept groups), k_se_walk (the rows),
// k_se_sum<S> + k_se_nodes<S> (up to rec_cap bs_node_request records for k_nodes_assume, counted in a.info[2]), k_se_groups; nothing when the
// call has no entries.  launch_seq_waiting: k_se_walk in its bs_seq_waiting_read form (wait_node pre-filled with -1)
struct SeqExpireDev;
void launch_seq_expire(hipStream_t stream, uint32_t S, const SeqExpireDev& a, const PodsDev& pd, const NodesDev& nd, bs_node_request* recs, uint32_t rec_cap);
void launch_seq_waiting(hipStream_t stream, const SeqExpireDev& a, int32_t* wait_node);

// the preemption victim search (tu_preempt.hip): k_preempt_scan<S> over scan_grid, then k_preempt_pick<S>, one wave per preemptor
struct PreemptDev;
void launch_preempt(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const PreemptDev& pe);

// the sequential preemption plan (tu_preempt.hip): k_pc_scan<S> over scan_grid, then k_pc_resolve<S>, one workgroup; and what
// BS_PREEMPT_APPLY launches after it: k_pc_nodes<S> (ndirty records into reqs), k_pc_boff<S> + k_pc_compact<S> when nw is set
struct CommitDev;
struct CompactDev;
void launch_preempt_commit(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe);
void launch_preempt_apply(hipStream_t stream, uint32_t S, const NodesDev& nd, const CommitDev& pe, uint32_t ndirty, uint32_t assume, bs_node_request* reqs,
                          const CompactDev* nw);
// bs_preempt_commit_gang's plan: k_pc_scan<S> as above, then k_gang_resolve<S> (the quorum of each gang's run, the rollback)
struct GangDev;
void launch_preempt_commit_gang(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe,
                                const GangDev& gd);

// the bound table's patch (tu_preempt.hip, bs_bound_apply.hpp): k_ba_scatter<S>, k_ba_mark<S>, k_ba_boff<S> (the new CSR into nw.boff),
// k_ba_merge<S> (one wave per node into nw; writes nothing when the error word is set)
struct BoundApplyDev;
void launch_bound_apply(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const CompactDev& nw);
// BS_BOUND_NODES, after the error word came back clear: k_ba_nodes<S> (one wave per node; the touched nodes' new request vectors as
// bs_node_request records for k_nodes_assume, counted in o.count)
struct BoundNodesReqDev;
void launch_bound_apply_nodes(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const BoundNodesReqDev& o);

// the bound table's remap after node-list surgery (tu_preempt.hip, bs_bound_nodes.hpp): k_bn_len<S>, k_bn_scan1<S> + k_bn_scan2<S> (the new
// CSR and the dropped ids' offsets, a.nblk blocks each), k_bn_move<S> (one wave per new node, and per removed node when ids are asked for)
struct BoundNodesDev;
void launch_bound_nodes(hipStream_t stream, uint32_t S, const BoundNodesDev& a);

// resident PodDisruptionBudgets (tu_preempt.hip, bs_pdb.hpp): k_pdb_allowed when a.count pairs are staged, then k_pdb_bits, one wave per node
// of the live table, rewrites its PDB byte column and per-node violating counts in place
struct PdbDev;
void launch_pdb(hipStream_t stream, const PdbDev& a);

}  // namespace bs
