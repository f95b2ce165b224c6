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

void launch_preempt(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const PreemptDev& pe) {
  lanes_wide(S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_preempt_scan<decltype(s)::value>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_preempt_pick<decltype(s)::value>), dim3(pe.q), dim3(64), 0, stream, nd, pd, pe);
  });
}

void launch_preempt_commit(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe) {
  lanes_wide(S, [&](auto s) {
    constexpr int V = decltype(s)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_scan<V>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_resolve<V>), dim3(1), dim3(pc_threads<V>()), 0, stream, nd, pd, pe);
  });
}

void launch_preempt_commit_gang(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe,
                                const GangDev& gd) {
  lanes_wide(S, [&](auto s) {
    constexpr int V = decltype(s)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_scan<V>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gang_resolve<V>), dim3(1), dim3(pc_threads<V>()), 0, stream, nd, pd, pe, gd);
  });
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
void launch_preempt_apply(hipStream_t stream, uint32_t S, const NodesDev& nd, const CommitDev& pe, uint32_t ndirty, uint32_t assume, bs_node_request* reqs,
                          const CompactDev* nw) {
  lanes_wide(S, [&](auto s) { launch_preempt_apply_s<decltype(s)::value>(stream, nd, pe, ndirty, assume, reqs, nw); });
}

template <int S>
static void launch_bound_apply_s(hipStream_t stream, const BoundApplyDev& a, const CompactDev& nw) {
  const uint32_t items = a.n_remove > a.n_insert ? a.n_remove : a.n_insert;
  if (a.b) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_scatter<S>), dim3((a.b + 255) / 256), dim3(256), 0, stream, a);
  if (items) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_mark<S>), dim3((items + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_boff<S>), dim3(1), dim3(1024), 0, stream, a, nw.boff);
  if (a.n) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_merge<S>), dim3((a.n + 3) / 4), dim3(256), 0, stream, a, nw);
}
void launch_bound_apply(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const CompactDev& nw) {
  lanes_wide(S, [&](auto s) { launch_bound_apply_s<decltype(s)::value>(stream, a, nw); });
}

void launch_bound_apply_nodes(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const BoundNodesReqDev& o) {
  if (a.n) lanes_wide(S, [&](auto s) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_nodes<decltype(s)::value>), dim3((a.n + 3) / 4), dim3(256), 0, stream, a, o); });
}

template <int S>
static void launch_bound_nodes_s(hipStream_t stream, const BoundNodesDev& a) {
  const uint32_t items = a.n1 > a.nrem ? a.n1 : a.nrem, waves = a.n1 + (a.dropped_cap ? a.nrem : 0u);
  if (items) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_len<S>), dim3((items + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_scan1<S>), dim3(a.nblk, 2), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_scan2<S>), dim3(a.nblk, 2), dim3(1024), 0, stream, a);
  if (waves) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_move<S>), dim3((waves + 3) / 4), dim3(256), 0, stream, a);
}
void launch_bound_nodes(hipStream_t stream, uint32_t S, const BoundNodesDev& a) {
  lanes_wide(S, [&](auto s) { launch_bound_nodes_s<decltype(s)::value>(stream, a); });
}

void launch_pdb(hipStream_t stream, const PdbDev& a) {
  if (a.count) hipLaunchKernelGGL(k_pdb_allowed, dim3((a.count + 255) / 256), dim3(256), 0, stream, a);
  if (a.n) hipLaunchKernelGGL(k_pdb_bits, dim3((a.n + 3) / 4), dim3(256), 0, stream, a);
}

}  // namespace bs
