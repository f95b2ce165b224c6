// tu_preempt.hip — translation unit of the preemption victim search (bs_preempt.hpp: k_preempt_scan / k_preempt_pick), of the
// sequential plans (bs_preempt_commit.hpp: k_pc_*), of the bound table's patch (bs_bound_apply.hpp: k_ba_*) and of its remap after node-list
// surgery (bs_bound_nodes.hpp: k_bn_*), one instantiation per scalar-lane count 0..BS_MAX_SCALARS, of the resident PodDisruptionBudgets
// (bs_pdb.hpp: k_pdb_*, no templates), and their launch wrappers; see tu_fast.hip for why.
#ifndef BS_UNITY
#define BS_TU_PREEMPT
#endif
#include "bs_preempt.hpp"
#include "bs_preempt_commit.hpp"
#include "bs_preempt_commit_gang.hpp"
#include "bs_bound_apply.hpp"
#include "bs_bound_nodes.hpp"
#include "bs_pdb.hpp"
#include "bs_launch.hpp"

namespace bs {

template <int S>
static void launch_preempt_s(hipStream_t stream, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const PreemptDev& pe) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_preempt_scan<S>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_preempt_pick<S>), dim3(pe.q), dim3(64), 0, stream, nd, pd, pe);
}

void launch_preempt(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const PreemptDev& pe) {
  switch (S) {
    case 0: launch_preempt_s<0>(stream, scan_grid, nd, pd, pe); break;
    case 1: launch_preempt_s<1>(stream, scan_grid, nd, pd, pe); break;
    case 2: launch_preempt_s<2>(stream, scan_grid, nd, pd, pe); break;
    case 3: launch_preempt_s<3>(stream, scan_grid, nd, pd, pe); break;
    case 4: launch_preempt_s<4>(stream, scan_grid, nd, pd, pe); break;
    case 5: launch_preempt_s<5>(stream, scan_grid, nd, pd, pe); break;
    case 6: launch_preempt_s<6>(stream, scan_grid, nd, pd, pe); break;
    case 7: launch_preempt_s<7>(stream, scan_grid, nd, pd, pe); break;
    case 8: launch_preempt_s<8>(stream, scan_grid, nd, pd, pe); break;
    case 9: launch_preempt_s<9>(stream, scan_grid, nd, pd, pe); break;
    case 10: launch_preempt_s<10>(stream, scan_grid, nd, pd, pe); break;
    case 11: launch_preempt_s<11>(stream, scan_grid, nd, pd, pe); break;
    default: launch_preempt_s<12>(stream, scan_grid, nd, pd, pe); break;
  }
}

template <int S>
static void launch_preempt_commit_s(hipStream_t stream, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_scan<S>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_resolve<S>), dim3(1), dim3(pc_threads<S>()), 0, stream, nd, pd, pe);
}

template <int S>
static void launch_preempt_commit_gang_s(hipStream_t stream, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe, const GangDev& gd) {
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_scan<S>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gang_resolve<S>), dim3(1), dim3(pc_threads<S>()), 0, stream, nd, pd, pe, gd);
}

template <int S>
static void launch_preempt_apply_s(hipStream_t stream, const NodesDev& nd, const CommitDev& pe, uint32_t ndirty, uint32_t assume, bs_node_request* reqs,
                                   const CompactDev* nw) {
  if (ndirty) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_nodes<S>), dim3((ndirty + 255) / 256), dim3(256), 0, stream, nd, pe, ndirty, assume, reqs);
  if (nw) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_boff<S>), dim3(1), dim3(1024), 0, stream, pe, nd.n, nw->boff);
    if (nd.n) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_compact<S>), dim3(nd.n), dim3(64), 0, stream, pe, *nw, nd.n);
  }
}

template <int S>
static void launch_bound_apply_s(hipStream_t stream, const BoundApplyDev& a, const CompactDev& nw) {
  const uint32_t items = a.n_remove > a.n_insert ? a.n_remove : a.n_insert;
  if (a.b) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_scatter<S>), dim3((a.b + 255) / 256), dim3(256), 0, stream, a);
  if (items) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_mark<S>), dim3((items + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_boff<S>), dim3(1), dim3(1024), 0, stream, a, nw.boff);
  if (a.n) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_merge<S>), dim3((a.n + 3) / 4), dim3(256), 0, stream, a, nw);
}

template <int S>
static void launch_bound_apply_nodes_s(hipStream_t stream, const BoundApplyDev& a, const BoundNodesReqDev& o) {
  if (a.n) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_nodes<S>), dim3((a.n + 3) / 4), dim3(256), 0, stream, a, o);
}

template <int S>
static void launch_bound_nodes_s(hipStream_t stream, const BoundNodesDev& a) {
  const uint32_t items = a.n1 > a.nrem ? a.n1 : a.nrem, waves = a.n1 + (a.dropped_cap ? a.nrem : 0u);
  if (items) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_len<S>), dim3((items + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_scan1<S>), dim3(a.nblk, 2), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_scan2<S>), dim3(a.nblk, 2), dim3(1024), 0, stream, a);
  if (waves) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_move<S>), dim3((waves + 3) / 4), dim3(256), 0, stream, a);
}

#define BS_PC_CASES(CALL) \
  switch (S) { \
    case 0: CALL(0); break; case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; \
    case 5: CALL(5); break; case 6: CALL(6); break; case 7: CALL(7); break; case 8: CALL(8); break; case 9: CALL(9); break; \
    case 10: CALL(10); break; case 11: CALL(11); break; default: CALL(12); break; \
  }

void launch_preempt_commit(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe) {
#define BS_PC_PLAN(s) launch_preempt_commit_s<s>(stream, scan_grid, nd, pd, pe)
  BS_PC_CASES(BS_PC_PLAN)
#undef BS_PC_PLAN
}

void launch_preempt_commit_gang(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe,
                                const GangDev& gd) {
#define BS_PC_GANG(s) launch_preempt_commit_gang_s<s>(stream, scan_grid, nd, pd, pe, gd)
  BS_PC_CASES(BS_PC_GANG)
#undef BS_PC_GANG
}

void launch_preempt_apply(hipStream_t stream, uint32_t S, const NodesDev& nd, const CommitDev& pe, uint32_t ndirty, uint32_t assume, bs_node_request* reqs,
                          const CompactDev* nw) {
#define BS_PC_APPLY(s) launch_preempt_apply_s<s>(stream, nd, pe, ndirty, assume, reqs, nw)
  BS_PC_CASES(BS_PC_APPLY)
#undef BS_PC_APPLY
}

void launch_bound_apply(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const CompactDev& nw) {
#define BS_BA_APPLY(s) launch_bound_apply_s<s>(stream, a, nw)
  BS_PC_CASES(BS_BA_APPLY)
#undef BS_BA_APPLY
}

void launch_bound_apply_nodes(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const BoundNodesReqDev& o) {
#define BS_BA_NODES(s) launch_bound_apply_nodes_s<s>(stream, a, o)
  BS_PC_CASES(BS_BA_NODES)
#undef BS_BA_NODES
}

void launch_bound_nodes(hipStream_t stream, uint32_t S, const BoundNodesDev& a) {
#define BS_BN_APPLY(s) launch_bound_nodes_s<s>(stream, a)
  BS_PC_CASES(BS_BN_APPLY)
#undef BS_BN_APPLY
}
#undef BS_PC_CASES

void launch_pdb(hipStream_t stream, const PdbDev& a) {
  if (a.count) hipLaunchKernelGGL(k_pdb_allowed, dim3((a.count + 255) / 256), dim3(256), 0, stream, a);
  if (a.n) hipLaunchKernelGGL(k_pdb_bits, dim3((a.n + 3) / 4), dim3(256), 0, stream, a);
}

}  // namespace bs
