// bs_seq_sample.hpp — the small arithmetic of rule F of include/bsched.h (bs_seq_run_scored_sampled, bs_seq_run_scored_nominated_sampled):
// upstream's numFeasibleNodesToFind (D9; v1.17.5, recalled, not vendored), the normalisation of K and of the start, visit position <-> node
// for a walk that starts at the cursor s and wraps, the cursor step, and the r-th set bit of a 64-bit mask (the lane of the (K+1)-th member
// inside a tile's ballot).  Plain C++ arithmetic, no HIP header: the kernel (bs_seq.hpp, seq_pick_sampled) and the host (tu_seq.hip) both
// include it, and tests/native/seq_sample_main.cpp compiles it alone under the host sanitizers.  Nothing here can overflow: every sum of
// two uint32 is formed in 64 bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BS_SAMPLE_FN __host__ __device__ inline
#else
#define BS_SAMPLE_FN inline
#endif

namespace bs {

constexpr uint32_t kSampleMinNodes = 100u;                   // upstream's minFeasibleNodesToFind
constexpr int64_t kSampleMinPercent = 5;                     // ... and minFeasibleNodesPercentageToFind
constexpr int64_t kSampleBasePercent = 50;

// D9: numFeasibleNodesToFind(n) under percentageOfNodesToScore = percentage; every division truncates
BS_SAMPLE_FN uint32_t sample_size(uint32_t n, int32_t percentage) {
  if (n < kSampleMinNodes || percentage >= 100) return n;
  int64_t a = percentage;
  if (a <= 0) {
    a = kSampleBasePercent - (int64_t)n / 125;
    if (a < kSampleMinPercent) a = kSampleMinPercent;
  }
  const int64_t k = (int64_t)n * a / 100;
  return k < (int64_t)kSampleMinNodes ? kSampleMinNodes : (uint32_t)k;
}

// K of rule F: 0 and everything from N on mean "all N"
BS_SAMPLE_FN uint32_t sample_k(uint32_t num_to_find, uint32_t N) { return (num_to_find == 0u || num_to_find >= N) ? N : num_to_find; }

// s_0 = start mod N (an empty list has the one cursor 0)
BS_SAMPLE_FN uint32_t sample_start(uint32_t start, uint32_t N) { return N ? start % N : 0u; }

// the node at visit position v of a walk that starts at s (s < N, v < N): (s + v) mod N
BS_SAMPLE_FN uint32_t sample_node(uint32_t s, uint32_t v, uint32_t N) {
  const uint64_t k = (uint64_t)s + (uint64_t)v;
  return (uint32_t)(k >= (uint64_t)N ? k - (uint64_t)N : k);
}

// ... and the visit position of node k (s < N, k < N)
BS_SAMPLE_FN uint32_t sample_pos(uint32_t s, uint32_t k, uint32_t N) { return k >= s ? k - s : (uint32_t)((uint64_t)k + (uint64_t)N - (uint64_t)s); }

// the cursor behind a pod that visited V nodes (s < N, V <= N): (s + V) mod N
BS_SAMPLE_FN uint32_t sample_step(uint32_t s, uint32_t V, uint32_t N) {
  if (!N) return 0u;
  const uint64_t k = (uint64_t)s + (uint64_t)V;
  return (uint32_t)(k >= (uint64_t)N ? k - (uint64_t)N : k);
}

BS_SAMPLE_FN uint32_t sample_popc64(uint64_t m) { return (uint32_t)__builtin_popcountll((unsigned long long)m); }

// the position of the r-th set bit of mask, r = 1 .. popcount(mask), counted from bit 0; 64 when the mask has fewer than r bits (or r == 0).
// Six halvings: the low half either holds the bit or its population is taken off r.
BS_SAMPLE_FN uint32_t sample_nth_bit(uint64_t mask, uint32_t r) {
  if (r == 0u || r > sample_popc64(mask)) return 64u;
  uint32_t pos = 0;
  for (uint32_t w = 32u; w; w >>= 1) {
    const uint64_t low = (mask >> pos) & ((1ull << w) - 1ull);
    const uint32_t c = sample_popc64(low);
    if (r > c) { r -= c; pos += w; }
  }
  return pos;
}

}  // namespace bs
