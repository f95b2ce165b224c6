// bs_lanes.hpp — how the scalar-lane count S of a context picks the instantiation of a lane-templated kernel: the three rules the host
// launches go by, each written once.  A rule calls f(Lane<V>{}) exactly once and returns what f returns (nothing, or the residency
// queries' int); the launch line inside f names its kernel as k<decltype(s)::value>.  Plain C++17, no HIP header: tests/native/lanes_main.cpp
// compiles it alone.  The fold is a chain of compares against constants, which the compiler turns into the jump table a switch would be.
#pragma once
#include <stdint.h>

#include <type_traits>
#include <utility>

#include "../../include/bsched.h"

namespace bs {

template <int V>
using Lane = std::integral_constant<int, V>;

// f(Lane<s>) where s is one of V..., f(Lane<ELSE>) where it is none of them
template <int ELSE, class F, int... V>
inline auto lanes_pick(uint32_t s, F&& f, std::integer_sequence<int, V...>) {
  using R = decltype(f(Lane<ELSE>{}));
  if constexpr (std::is_void_v<R>) {
    if (!((s == (uint32_t)V && (f(Lane<V>{}), true)) || ...)) f(Lane<ELSE>{});
  } else {
    R r{};
    if (!((s == (uint32_t)V && (r = f(Lane<V>{}), true)) || ...)) r = f(Lane<ELSE>{});
    return r;
  }
}

// the wide families (one instantiation per lane count a context can have): V = min(S, BS_MAX_SCALARS)
static_assert(BS_MAX_SCALARS == 12, "a new bound adds an instantiation to every wide family: look at their registers and scratch (tools/kernel_resources.py)");
template <class F>
inline auto lanes_wide(uint32_t s, F&& f) {
  return lanes_pick<BS_MAX_SCALARS>(s, f, std::make_integer_sequence<int, BS_MAX_SCALARS>{});
}

// what the other two rules unroll up to
constexpr int kLanesUnrolled = 4;

// the narrow families: V = S up to kLanesUnrolled, beyond that -1, the generic-lane instantiation (a loop over the lanes)
template <class F>
inline auto lanes_narrow(uint32_t s, F&& f) {
  return lanes_pick<-1>(s, f, std::make_integer_sequence<int, kLanesUnrolled + 1>{});
}

// the families that have no generic-lane instantiation: V = min(S, kLanesUnrolled).  Their callers never come with more lanes
// (step_a_possible, and launch_b_plan's test for the transposed one-launch form, both in bs_step_geom.hpp); the clamp only keeps a stray S inside the set.
template <class F>
inline auto lanes_clamped(uint32_t s, F&& f) {
  return lanes_pick<kLanesUnrolled>(s, f, std::make_integer_sequence<int, kLanesUnrolled>{});
}

}  // namespace bs
