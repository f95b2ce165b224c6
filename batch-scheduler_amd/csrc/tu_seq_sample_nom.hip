// tu_seq_sample_nom.hip — translation unit of the sequential pass under rule F over rule SP (include/bsched.h:
// bs_seq_run_scored_nominated_sampled): the thirteen fixed-lane instantiations k_seq_sampled_nom<TS>, TS = 0 .. BS_MAX_SCALARS, of bs_seq.hpp
// and their launch wrapper, which tu_seq.hip's entry point calls.  A unit of its own, and nothing but the kernels, for the reason
// tu_seq_nom.hip states (profiles/seq_sampled_isa_diff.txt).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_seq.hpp"
#include "bs_lanes.hpp"

namespace bs {

void launch_seq_sampled_nominated(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq,
                                  const SeqParams& prm, const SeqNom& nom, const SeqScore& sco, const SeqSample& smp) {
  lanes_wide(S, [&](auto s) {
    constexpr int TS = decltype(s)::value;
    void (*kn)(PodsDev, GroupsDev, NodesDev, SeqDev, SeqParams, SeqNom, SeqScore, SeqSample) = &k_seq_sampled_nom<TS>;
    // static LDS + the key window + the NOM-only, the scored-only and the sampled-only state can exceed the default 64 KB of dynamic LDS
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seq_sampled_nom<TS>), dim3(1), dim3(kSeqBlock), lds, stream, pd, gr, nd, sq, prm, nom, sco, smp);
  });
}

}  // namespace bs
