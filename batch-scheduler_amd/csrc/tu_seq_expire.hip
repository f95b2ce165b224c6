// tu_seq_expire.hip — translation unit of the Permit timeout that undoes the pass's waiting gangs (bs_seq_expire.hpp: k_se_*, the two
// lane-templated kernels once per scalar-lane count 0..BS_MAX_SCALARS) and its launch wrappers.  A unit of its own, not tu_seq.hip: with
// these kernels in the pass's unit one instantiation of k_seq_pass came out with other instructions (profiles/seq_expire_isa_diff.txt).
// Like tu_seq.hip it emits none of the shared headers' non-template kernels (BS_TU_SEQ, bs_common.hpp).
#ifndef BS_UNITY
#define BS_TU_SEQ
#endif
#include "bs_seq_expire.hpp"
#include "bs_launch.hpp"

namespace bs {

void launch_seq_expire(hipStream_t stream, uint32_t S, const SeqExpireDev& a, const PodsDev& pd, const NodesDev& nd, bs_node_request* recs, uint32_t rec_cap) {
  if (!a.M) return;
  const uint32_t nblk = (a.M + kSeBlock - 1) / kSeBlock;
  hipLaunchKernelGGL(k_se_scan1, dim3(nblk), dim3(kSeBlock), 0, stream, a);
  hipLaunchKernelGGL(k_se_scan2, dim3(nblk), dim3(kSeBlock), 0, stream, a);
  hipLaunchKernelGGL(k_se_walk, dim3((a.M + 255) / 256), dim3(256), 0, stream, a, (int32_t*)nullptr);
  if (a.P && rec_cap) lanes_wide(S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_se_sum<decltype(s)::value>), dim3((a.P + 255) / 256), dim3(256), 0, stream, a, pd);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_se_nodes<decltype(s)::value>), dim3((rec_cap + 255) / 256), dim3(256), 0, stream, a, nd.req, nd.rpres, nd.stride, recs);
  });
  hipLaunchKernelGGL(k_se_groups, dim3((a.M + 255) / 256), dim3(256), 0, stream, a);
}

void launch_seq_waiting(hipStream_t stream, const SeqExpireDev& a, int32_t* wait_node) {
  if (a.G) hipLaunchKernelGGL(k_se_walk, dim3((a.G + 255) / 256), dim3(256), 0, stream, a, wait_node);
}

}  // namespace bs
