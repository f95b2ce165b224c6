// Gang-aligned pod ranges of the whole-step launch (k_fast_step_a<TS, true>, bs_fast.hpp), computed on the host when the queue arrives (bs_pods_load).
// Plain C++: the CPU tests compile it on its own (tests/test_pod_ranges_cpu.py).
//
// A gang's pods sit next to each other in a real queue (the reference's Less: priority, then the group's timestamp).  A CUT is a queue position where every
// gang that started before it has also ended; pods without a group do not constrain cuts.  From s, a range ends at the largest cut c <= s + cap, or at
// s + cap when there is none.  A gang is LOCAL when all of its pods fall inside one range: the pod block of that range counts it and closes its quorum in
// LDS (tally_tail_whole), with no global atomic.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace bs {

struct PodRanges {
  std::vector<uint32_t> start;   // [ranges + 1] first pod of each range, then P
  std::vector<uint32_t> lfirst;  // [P] queue position of the first pod of the pod's gang when the gang is local, 0xFFFFFFFF otherwise
  std::vector<uint8_t> glocal;   // [group ids below the bound] 1: the gang is local (arm_tally leaves its counters to the closing block)
};

// group[i] < 0: no group.  Group ids at or above `gbound` are treated as no group (never local: the kernels' returning-atomic path takes them).
inline void pod_ranges(const int32_t* group, uint32_t P, uint32_t cap, uint32_t gbound, PodRanges& out) {
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  auto gid = [&](uint32_t i) -> uint32_t { return group[i] >= 0 && (uint32_t)group[i] < gbound ? (uint32_t)group[i] : kNone; };
  uint32_t ng = 0;
  for (uint32_t i = 0; i < P; ++i)
    if (gid(i) != kNone) ng = std::max(ng, gid(i) + 1u);
  std::vector<uint32_t> first(ng, kNone), last(ng, 0u);
  for (uint32_t i = 0; i < P; ++i) {
    const uint32_t g = gid(i);
    if (g == kNone) continue;
    if (first[g] == kNone) first[g] = i;
    last[g] = i;
  }
  // prevcut[x]: the largest cut <= x (0 and P are cuts)
  std::vector<uint32_t> prevcut((size_t)P + 1u, 0u);
  uint32_t open_end = 0;                              // max(last + 1) over the gangs of the pods before the position
  for (uint32_t c = 1; c <= P; ++c) {
    const uint32_t g = gid(c - 1u);
    if (g != kNone) open_end = std::max(open_end, last[g] + 1u);
    prevcut[c] = open_end <= c ? c : prevcut[c - 1u];
  }
  out.start.clear();
  std::vector<uint32_t> rid((size_t)P, 0u);
  for (uint32_t s = 0; s < P;) {
    const uint32_t e = std::min<uint32_t>(P, s + cap);
    uint32_t c = prevcut[e];
    if (c <= s) c = e;
    for (uint32_t i = s; i < c; ++i) rid[i] = (uint32_t)out.start.size();
    out.start.push_back(s);
    s = c;
  }
  out.start.push_back(P);
  out.glocal.assign(ng, 0u);
  for (uint32_t g = 0; g < ng; ++g)
    if (first[g] != kNone && rid[first[g]] == rid[last[g]]) out.glocal[g] = 1u;
  out.lfirst.assign(P, kNone);
  for (uint32_t i = 0; i < P; ++i) {
    const uint32_t g = gid(i);
    if (g != kNone && out.glocal[g]) out.lfirst[i] = first[g];
  }
}

}  // namespace bs
