// tu_preempt.hip — translation unit of the preemption victim search (bs_preempt.hpp: k_preempt_scan / k_preempt_pick, one
// instantiation per scalar-lane count 0..BS_MAX_SCALARS) and its launch wrapper; see tu_fast.hip for why.
#ifndef BS_UNITY
#define BS_TU_PREEMPT
#endif
#include "bs_preempt.hpp"
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

}  // namespace bs
