// tu_fast.hip — translation unit of the steady-state chain's second launch: the scan / Filter role kernels of bs_fast.hpp and
// bs_filter_t.hpp (13 scalar-lane instantiations each) and their launch wrappers.  A translation unit of its own so that the library
// builds in parallel and a change to one kernel family recompiles that family only (bs_launch.hpp is the interface; -DBS_UNITY, the
// probe builds, includes this file into bsched.hip instead).
#ifndef BS_UNITY
#define BS_TU_FAST
#endif
#include "bs_fast.hpp"
#include "bs_launch.hpp"

#include <algorithm>

namespace bs {

void launch_fast_b(const FastLaunch& c, dim3 grid, const PodsDev& pd, const NodesDev& nd, const BatchDev& bt, const BatchParams& prm, uint32_t nseg,
                          uint32_t scan_blocks) {
  lanes_wide(c.S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_scan_filter<decltype(s)::value>), grid, dim3(256), 0, c.stream, pd, nd, bt, prm, c.M, nseg, scan_blocks,
                       c.filter_waves, c.filter_slots_cap);
  });
}
void launch_fast_scan(const FastLaunch& c, dim3 grid, const BatchDev& bt, const BatchParams& prm, uint32_t nseg) {
  lanes_wide(c.S, [&](auto s) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_scan<decltype(s)::value>), grid, dim3(256), 0, c.stream, bt, prm, c.M, nseg); });
}
void launch_fast_bt(const FastLaunch& c, dim3 grid, const NodesDev& nd, const BatchDev& bt, const BatchParams& prm, uint32_t nseg, uint32_t scan_blocks) {
  // S <= 4 only (run_fast sends wider contexts through k_fast_scan + k_fast_filter_t): beyond that the two roles in one kernel run out
  // of SGPRs and the instantiation reserves scratch memory (36 bytes at S = 5, tools/kernel_resources.py), which every launch pays for
  lanes_clamped(c.S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_scan_filter_t<decltype(s)::value>), grid, dim3(256), 0, c.stream, nd, bt, prm, c.M, nseg, scan_blocks,
                       c.filter_split ? c.filter_split : c.filter_waves, c.filter_slots_cap, (c.tp_filter == 7u ? 1u : 0u) | (c.filter_split ? 2u : 0u));
  });
}
void launch_fast_filter(const FastLaunch& c, dim3 grid, const PodsDev& pd, const NodesDev& nd, const BatchDev& bt, const BatchParams& prm) {
  switch (c.tp_filter) {
    case 1: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_filter<4, true>), grid, dim3(256), 0, c.stream, pd, nd, bt, prm, c.filter_waves, c.filter_slots_cap); break;
    case 2: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_filter<2, true>), grid, dim3(256), 0, c.stream, pd, nd, bt, prm, c.filter_waves, c.filter_slots_cap); break;
    case 3: hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_filter<2, false>), grid, dim3(256), 0, c.stream, pd, nd, bt, prm, c.filter_waves, c.filter_slots_cap); break;
    case 4: hipLaunchKernelGGL(k_fast_filter_w7, grid, dim3(256), 0, c.stream, pd, nd, bt, prm, c.filter_waves, c.filter_slots_cap); break;
    default: hipLaunchKernelGGL(k_fast_filter_t, grid, dim3(256), 0, c.stream, nd, bt, prm, c.filter_split ? c.filter_split : c.filter_waves, c.filter_slots_cap, c.filter_split ? 1u : 0u); break;
  }
}
// How many blocks of a launch that waits inside itself the chip holds at once (occupancy API, minus one block per CU: the API can be one
// high, MI355X_MICROARCH.md "Residency").  Such a launch is only taken when its whole grid fits: then no producer block can be
// waiting for a slot that a spinning final block occupies, whatever order the dispatcher hands blocks out in.
template <class K>
static int blocks_resident(const FastLaunch& c, K kernel, int block) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, 0) != hipSuccess || per_cu <= 0) return 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c.device) != hipSuccess) return 0;
  return std::max(0, per_cu - 1) * prop.multiProcessorCount;
}
int fused_residency_query(const FastLaunch& c) {
  return lanes_wide(c.S, [&](auto s) { return blocks_resident(c, k_fast_scan_filter_final<decltype(s)::value>, 256); });
}
void launch_fast_bc(const FastLaunch& c, dim3 grid, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const BatchDev& b, const BatchDev& bt,
                           const BatchParams& prm, uint32_t nseg, uint32_t scan_blocks, uint32_t filter_blocks) {
  lanes_wide(c.S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_scan_filter_final<decltype(s)::value>), grid, dim3(256), 0, c.stream, pd, gr, nd, b, bt, prm, c.M, nseg,
                       scan_blocks, filter_blocks, c.filter_waves, c.filter_slots_cap, cdiv(c.P, kTblChunk));
  });
}

void launch_fast_step_a(const FastLaunch& c, dim3 grid, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const BatchDev& b, const BatchDev& bt,
                        const BatchParams& prm, const TableDesc* forced, uint32_t nchunks, uint32_t query_blocks, uint32_t nshares, uint32_t filter_blocks,
                        uint32_t tk_pods0, uint32_t tk_tab0, uint32_t param_blocks, const int64_t* ckeys, const uint32_t* cpres, uint32_t kcap,
                        uint32_t whole, uint32_t tk_p1, uint32_t tk_done, uint32_t forced_cls) {
  lanes_clamped(c.S, [&](auto s) {
    auto launch = [&](auto whole_step) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fast_step_a<decltype(s)::value, decltype(whole_step)::value>), grid, dim3(kTblChunk), 0, c.stream, pd, gr, nd, b, bt,
                         prm, forced, nchunks, query_blocks, nshares, filter_blocks, c.filter_waves, c.filter_slots_cap, tk_pods0, tk_tab0, param_blocks,
                         ckeys, cpres, kcap, tk_p1, tk_done, forced_cls);
    };
    if (whole) launch(std::true_type{});
    else launch(std::false_type{});
  });
}
int step_a_residency_query(const FastLaunch& c, bool whole) {
  return lanes_clamped(c.S, [&](auto s) {
    constexpr int TS = decltype(s)::value;
    return whole ? blocks_resident(c, k_fast_step_a<TS, true>, (int)kTblChunk) : blocks_resident(c, k_fast_step_a<TS, false>, (int)kTblChunk);
  });
}

}  // namespace bs
