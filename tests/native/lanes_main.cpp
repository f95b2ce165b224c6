// Driver of csrc/bs_lanes.hpp for tests/test_lanes_cpu.py, compiled alone with g++ (ASan + UBSan).  For every S in 0..40 one line:
//   S  wide-constant wide-calls  narrow-constant narrow-calls  clamped-constant clamped-calls  value-returned-by-the-wide-rule
// The first three callables return nothing (the launches' form), the last one returns an int (the residency queries' form).
#include <cstdio>

#include "bs_lanes.hpp"

int main() {
  for (uint32_t S = 0; S <= 40; ++S) {
    int got[3] = {-99, -99, -99}, calls[3] = {0, 0, 0};
    bs::lanes_wide(S, [&](auto s) { got[0] = decltype(s)::value; calls[0]++; });
    bs::lanes_narrow(S, [&](auto s) { got[1] = decltype(s)::value; calls[1]++; });
    bs::lanes_clamped(S, [&](auto s) { got[2] = decltype(s)::value; calls[2]++; });
    const int ret = bs::lanes_wide(S, [&](auto s) { return 1000 + decltype(s)::value; });
    const int ret_n = bs::lanes_narrow(S, [&](auto s) { return 1000 + decltype(s)::value; });
    const int ret_c = bs::lanes_clamped(S, [&](auto s) { return 1000 + decltype(s)::value; });
    std::printf("%u %d %d %d %d %d %d %d %d %d\n", S, got[0], calls[0], got[1], calls[1], got[2], calls[2], ret, ret_n, ret_c);
  }
  return 0;
}
