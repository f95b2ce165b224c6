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

template <int S>
static void launch_seq_expire_s(hipStream_t stream, const SeqExpireDev& a, const PodsDev& pd, const NodesDev& nd, bs_node_request* recs, uint32_t rec_cap) {
  const uint32_t nblk = (a.M + kSeBlock - 1) / kSeBlock;
  hipLaunchKernelGGL(k_se_scan1, dim3(nblk), dim3(kSeBlock), 0, stream, a);
  hipLaunchKernelGGL(k_se_scan2, dim3(nblk), dim3(kSeBlock), 0, stream, a);
  hipLaunchKernelGGL(k_se_walk, dim3((a.M + 255) / 256), dim3(256), 0, stream, a, (int32_t*)nullptr);
  if (a.P && rec_cap) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_se_sum<S>), dim3((a.P + 255) / 256), dim3(256), 0, stream, a, pd);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_se_nodes<S>), dim3((rec_cap + 255) / 256), dim3(256), 0, stream, a, nd.req, nd.rpres, nd.stride, recs);
  }
  hipLaunchKernelGGL(k_se_groups, dim3((a.M + 255) / 256), dim3(256), 0, stream, a);
}

void launch_seq_expire(hipStream_t stream, uint32_t S, const SeqExpireDev& a, const PodsDev& pd, const NodesDev& nd, bs_node_request* recs, uint32_t rec_cap) {
  if (!a.M) return;
  switch (S) {
    case 0: launch_seq_expire_s<0>(stream, a, pd, nd, recs, rec_cap); break;
    case 1: launch_seq_expire_s<1>(stream, a, pd, nd, recs, rec_cap); break;
    case 2: launch_seq_expire_s<2>(stream, a, pd, nd, recs, rec_cap); break;
    case 3: launch_seq_expire_s<3>(stream, a, pd, nd, recs, rec_cap); break;
    case 4: launch_seq_expire_s<4>(stream, a, pd, nd, recs, rec_cap); break;
    case 5: launch_seq_expire_s<5>(stream, a, pd, nd, recs, rec_cap); break;
    case 6: launch_seq_expire_s<6>(stream, a, pd, nd, recs, rec_cap); break;
    case 7: launch_seq_expire_s<7>(stream, a, pd, nd, recs, rec_cap); break;
    case 8: launch_seq_expire_s<8>(stream, a, pd, nd, recs, rec_cap); break;
    case 9: launch_seq_expire_s<9>(stream, a, pd, nd, recs, rec_cap); break;
    case 10: launch_seq_expire_s<10>(stream, a, pd, nd, recs, rec_cap); break;
    case 11: launch_seq_expire_s<11>(stream, a, pd, nd, recs, rec_cap); break;
    default: launch_seq_expire_s<12>(stream, a, pd, nd, recs, rec_cap); break;
  }
}

void launch_seq_waiting(hipStream_t stream, const SeqExpireDev& a, int32_t* wait_node) {
  if (a.G) hipLaunchKernelGGL(k_se_walk, dim3((a.G + 255) / 256), dim3(256), 0, stream, a, wait_node);
}

}  // namespace bs
