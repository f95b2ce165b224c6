// Stand-alone driver of rule P (csrc/bs_seq_score.hpp; tests/test_seq_scored_cpu.py builds it under ASan + UBSan — signed overflow in the
// sum requested + request or in a `* 100` would be a report): one case per line, one answer line per case.  q = the node's requested value,
// p = the pod's request; R = q + p as the kernel forms it (score_wadd).
//   A0 q0 p0 A1 q1 p1 w_least w_most w_balanced   ->   "R0 R1 least most balanced total"
#include <cinttypes>
#include <cstdio>

#include "bs_seq_score.hpp"

int main() {
  int64_t A0, q0, p0, A1, q1, p1;
  unsigned wl, wm, wb;
  while (std::scanf("%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %u %u %u", &A0, &q0, &p0, &A1, &q1, &p1, &wl, &wm, &wb) == 9) {
    const int64_t R0 = bs::score_wadd(q0, p0), R1 = bs::score_wadd(q1, p1);
    std::printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %u\n", R0, R1, bs::score_least(A0, R0, A1, R1), bs::score_most(A0, R0, A1, R1),
                bs::score_balanced(A0, R0, A1, R1), bs::score_total(A0, R0, A1, R1, wl, wm, wb));
  }
  return 0;
}
