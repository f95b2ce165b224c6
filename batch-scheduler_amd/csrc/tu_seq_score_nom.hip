// tu_seq_score_nom.hip — translation unit of the sequential pass under rules S and P at once (include/bsched.h, rule SP:
// bs_seq_run_scored_nominated): the thirteen fixed-lane instantiations k_seq_sp<TS>, TS = 0 .. BS_MAX_SCALARS, of bs_seq.hpp and
// their launch wrapper, which tu_seq.hip's entry point calls.  A unit of its own, and nothing but the kernels, for the reason
// tu_seq_nom.hip states: what else a module holds moves the optimiser's choices, and the kernels of bs_seq_run, bs_seq_run_nominated and
// bs_seq_run_scored stay instruction-identical (profiles/seq_scored_nominated_isa_diff.txt).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_seq.hpp"
#include "bs_lanes.hpp"

namespace bs {

void launch_seq_scored_nominated(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq,
                                 const SeqParams& prm, const SeqNom& nom, const SeqScore& sco) {
  lanes_wide(S, [&](auto s) {
    constexpr int TS = decltype(s)::value;
    void (*kn)(PodsDev, GroupsDev, NodesDev, SeqDev, SeqParams, SeqNom, SeqScore) = &k_seq_sp<TS>;
    // static LDS + the key window + the NOM-only and the scored-only state can exceed the default 64 KB of dynamic LDS
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seq_sp<TS>), dim3(1), dim3(kSeqBlock), lds, stream, pd, gr, nd, sq, prm, nom, sco);
  });
}

}  // namespace bs
