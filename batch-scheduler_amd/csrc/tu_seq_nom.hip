// tu_seq_nom.hip — translation unit of the sequential pass under rule S (include/bsched.h, bs_seq_run_nominated): the six NOM instantiations
// k_seq_pass<TS, true> of bs_seq.hpp and their launch wrapper, which tu_seq.hip's entry point calls.  A unit of its own, and nothing but
// the kernels: with the twelve instantiations in ONE unit the flag-less k_seq_pass<4> came out as other instructions than it was (the
// optimiser's choices in a kernel depend on what else the module holds), and bs_seq_run's kernels stay instruction-identical
// (profiles/seq_nominated_isa_diff.txt).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_seq.hpp"
#include "bs_lanes.hpp"

namespace bs {

void launch_seq_nominated(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq, const SeqParams& prm,
                          const SeqNom& nom) {
  lanes_narrow(S, [&](auto s) {
    constexpr int TS = decltype(s)::value;
    void (*kn)(PodsDev, GroupsDev, NodesDev, SeqDev, SeqParams, SeqNom) = &k_seq_pass<TS, true>;
    // static LDS + the key window + the NOM-only state can exceed the default 64 KB of dynamic LDS
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_seq_pass<TS, true>), dim3(1), dim3(kSeqBlock), lds, stream, pd, gr, nd, sq, prm, nom);
  });
}

}  // namespace bs
