// bs_seq_score.hpp — rule P of include/bsched.h (bs_seq_run_scored): the score of ONE node for ONE pod, from the cpu and memory lanes alone.
// Upstream's default priorities of v1.17.5 (recalled, not vendored): LeastRequested, MostRequested, BalancedResourceAllocation, each 0..100,
// weighted and summed.  A0 / A1 are the node's allocatable cpu / memory, R0 / R1 the requests on it WITH the pod (the caller's wrapping sum).
// Plain C++ arithmetic, no HIP header: the kernel (bs_seq.hpp, seq_pick_scored) calls score_total, and tests/native/seq_score_main.cpp
// compiles this file alone under the host sanitizers.  Nothing here can overflow: a lane outside the domain never reaches the
// multiplication, and inside it A < 2^53 keeps (A - R) * 100 and R * 100 below 2^60 and both conversions to double exact.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BS_SCORE_FN __host__ __device__ inline
#else
#define BS_SCORE_FN inline
#endif

namespace bs {

constexpr uint32_t kScoreWeightMax = 65536u;                 // BS_SCORE_WEIGHT_MAX: total <= 3 * 100 * 65536 < 2^32
constexpr int64_t kScoreDomain = (int64_t)1 << 53;

// requested + request as Go adds them: int64, wrapping
BS_SCORE_FN int64_t score_wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }

// upstream answers 0 for capacity == 0 and for requested > capacity; negative, wrapped and huge values are outside as well
BS_SCORE_FN bool score_in_domain(int64_t A, int64_t R) { return A > 0 && A < kScoreDomain && R >= 0 && R <= A; }

BS_SCORE_FN int64_t score_least_lane(int64_t A, int64_t R) { return score_in_domain(A, R) ? ((A - R) * 100) / A : 0; }
BS_SCORE_FN int64_t score_most_lane(int64_t A, int64_t R) { return score_in_domain(A, R) ? (R * 100) / A : 0; }
BS_SCORE_FN double score_frac_lane(int64_t A, int64_t R) { return score_in_domain(A, R) ? (double)R / (double)A : 1.0; }

BS_SCORE_FN int64_t score_least(int64_t A0, int64_t R0, int64_t A1, int64_t R1) { return (score_least_lane(A0, R0) + score_least_lane(A1, R1)) / 2; }
BS_SCORE_FN int64_t score_most(int64_t A0, int64_t R0, int64_t A1, int64_t R1) { return (score_most_lane(A0, R0) + score_most_lane(A1, R1)) / 2; }
// binary64, every operation rounded on its own (the build has -ffp-contract=off -fno-fast-math)
BS_SCORE_FN int64_t score_balanced(int64_t A0, int64_t R0, int64_t A1, int64_t R1) {
  const double f0 = score_frac_lane(A0, R0), f1 = score_frac_lane(A1, R1);
  if (f0 >= 1.0 || f1 >= 1.0) return 0;
  const double d = f0 - f1;
  return (int64_t)((1.0 - (d < 0.0 ? -d : d)) * 100.0);     // in [0, 100]: truncation toward zero
}

BS_SCORE_FN uint32_t score_total(int64_t A0, int64_t R0, int64_t A1, int64_t R1, uint32_t w_least, uint32_t w_most, uint32_t w_balanced) {
  uint64_t t = 0;                                            // (a weight of 0 skips its term: the value is the same, the divisions are not paid)
  if (w_least) t += (uint64_t)w_least * (uint64_t)score_least(A0, R0, A1, R1);
  if (w_most) t += (uint64_t)w_most * (uint64_t)score_most(A0, R0, A1, R1);
  if (w_balanced) t += (uint64_t)w_balanced * (uint64_t)score_balanced(A0, R0, A1, R1);
  return (uint32_t)t;
}

}  // namespace bs
