// tu_seq_score.hip — translation unit of the sequential pass under rule P (include/bsched.h, bs_seq_run_scored): the thirteen
// fixed-lane instantiations k_seq_scored<TS>, TS = 0 .. BS_MAX_SCALARS, of bs_seq.hpp (why there is no generic-lane one is said there) and
// their launch wrapper, which tu_seq.hip's entry point calls.  A unit of its own, and nothing but
// the kernels, for the reason tu_seq_nom.hip states: what else a module holds moves the optimiser's choices, and the twelve kernels of
// bs_seq_run and bs_seq_run_nominated stay instruction-identical (profiles/seq_scored_isa_diff.txt).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_seq.hpp"
#include "bs_lanes.hpp"

namespace bs {

void launch_seq_scored(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq, const SeqParams& prm,
                       const SeqScore& sco) {
  lanes_wide(S, [&](auto s) {
    constexpr int TS = decltype(s)::value;
    static_assert(kSeqScoredFullLanes == kLanesUnrolled, "the full form covers the lane counts the other pass kernels unroll");
    void (*kn)(PodsDev, GroupsDev, NodesDev, SeqDev, SeqParams, SeqScore) = &k_seq_scored<TS>;
    // static LDS + the key window + the scored-only state can exceed the default 64 KB of dynamic LDS
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seq_scored<TS>), dim3(1), dim3(kSeqBlock), lds, stream, pd, gr, nd, sq, prm, sco);
  });
}

}  // namespace bs
