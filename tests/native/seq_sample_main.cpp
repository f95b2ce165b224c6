// Stand-alone driver of rule F's arithmetic (csrc/bs_seq_sample.hpp; tests/test_seq_sampled_cpu.py builds it under ASan + UBSan — an
// overflow in a sum of two uint32, a shift by 64 in the r-th-set-bit helper would be a report).  It checks by itself, against loops that state
// the same thing the slow way, and prints one line per family; any mismatch is printed and ends the program with status 1.  One command per
// input line on top of that, for the test's own vectors:
//   size n percentage      ->  bs::sample_size(n, percentage)
//   walk s N               ->  "node(0) node(1) node(N-1) pos(node(1)) step(N)" of a walk from s % N
//   bit mask_hex r         ->  bs::sample_nth_bit(mask, r)
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "bs_seq_sample.hpp"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("MISMATCH " __VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

static uint32_t slow_nth_bit(uint64_t mask, uint32_t r) {
  if (r == 0) return 64;
  for (uint32_t b = 0; b < 64; ++b)
    if ((mask >> b) & 1u) { if (--r == 0) return b; }
  return 64;
}

static void self_check() {
  // D9: upstream's own table, and the edges of every branch
  struct { int32_t pct; uint32_t n, want; } d9[] = {{0, 10, 10}, {40, 10, 10}, {0, 1000, 420}, {40, 1000, 400}, {0, 6000, 300}, {40, 6000, 2400}, {0, 5000, 500},
                                                     {0, 99, 99}, {0, 100, 100}, {100, 5000, 5000}, {99, 100, 100}, {5, 20000, 1000}, {-1, 20000, 1000},
                                                     {0, 4294967295u, 214748364u}, {1, 4294967295u, 42949672u}};
  for (auto& v : d9) CHECK(bs::sample_size(v.n, v.pct) == v.want, "sample_size(%u, %d) = %u, want %u", v.n, v.pct, bs::sample_size(v.n, v.pct), v.want);
  // K and the start
  CHECK(bs::sample_k(0, 50) == 50 && bs::sample_k(50, 50) == 50 && bs::sample_k(51, 50) == 50 && bs::sample_k(49, 50) == 49 && bs::sample_k(1, 1) == 1 &&
        bs::sample_k(7, 0) == 0 && bs::sample_k(4294967295u, 4294967295u) == 4294967295u, "sample_k");
  CHECK(bs::sample_start(7, 0) == 0 && bs::sample_start(7, 7) == 0 && bs::sample_start(15, 8) == 7 && bs::sample_start(4294967295u, 4294967294u) == 1, "sample_start");
  // the rotation: a walk from s visits every node once, positions and nodes are inverse, the step wraps
  const uint32_t Ns[] = {1, 2, 63, 64, 65, 129, 513};
  for (uint32_t N : Ns) {
    const uint32_t ss[] = {0, 1, 63, 64, N - 1};
    for (uint32_t s0 : ss) {
      const uint32_t s = bs::sample_start(s0, N);
      uint64_t sum = 0;
      for (uint32_t v = 0; v < N; ++v) {
        const uint32_t k = bs::sample_node(s, v, N);
        CHECK(k < N && k == (uint32_t)(((uint64_t)s + v) % N), "sample_node(%u, %u, %u) = %u", s, v, N, k);
        CHECK(bs::sample_pos(s, k, N) == v, "sample_pos(%u, %u, %u) = %u, want %u", s, k, N, bs::sample_pos(s, k, N), v);
        sum += k;
      }
      CHECK(sum == (uint64_t)N * (N - 1) / 2, "a walk from %u over %u nodes visits every node once", s, N);
      for (uint32_t V = 0; V <= N; ++V) CHECK(bs::sample_step(s, V, N) == (uint32_t)(((uint64_t)s + V) % N), "sample_step(%u, %u, %u)", s, V, N);
    }
  }
  // ... at the top of uint32 (the sums are formed in 64 bits)
  const uint32_t big = 4294967295u;
  CHECK(bs::sample_node(big - 1, big - 1, big) == big - 2 && bs::sample_pos(big - 1, 0, big) == 1 && bs::sample_step(big - 1, big, big) == big - 1 &&
        bs::sample_step(0, 0, 0) == 0, "the top of uint32");
  // the r-th set bit: all ones, single bits, alternating masks, nothing to find
  const uint64_t ones = ~0ull, even = 0x5555555555555555ull, odd = 0xAAAAAAAAAAAAAAAAull;
  for (uint32_t r = 0; r <= 65; ++r) {
    CHECK(bs::sample_nth_bit(ones, r) == slow_nth_bit(ones, r), "nth_bit(ones, %u)", r);
    CHECK(bs::sample_nth_bit(even, r) == slow_nth_bit(even, r), "nth_bit(even, %u)", r);
    CHECK(bs::sample_nth_bit(odd, r) == slow_nth_bit(odd, r), "nth_bit(odd, %u)", r);
    CHECK(bs::sample_nth_bit(0, r) == 64, "nth_bit(0, %u)", r);
  }
  for (uint32_t b = 0; b < 64; ++b) {
    CHECK(bs::sample_nth_bit(1ull << b, 1) == b && bs::sample_nth_bit(1ull << b, 2) == 64, "nth_bit(1 << %u)", b);
    CHECK(bs::sample_nth_bit(ones << b, 1) == b && bs::sample_nth_bit(ones >> b, 64 - b) == 63 - b, "nth_bit of a run from / up to bit %u", b);
  }
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (int it = 0; it < 2000; ++it) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const uint32_t r = (uint32_t)(x % 66);
    CHECK(bs::sample_nth_bit(x, r) == slow_nth_bit(x, r), "nth_bit(%016" PRIx64 ", %u)", x, r);
  }
  std::printf("self-check %s\n", failures ? "FAILED" : "ok");
}

int main() {
  self_check();
  char cmd[16];
  while (std::scanf("%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "size")) {
      uint32_t n; int32_t pct;
      if (std::scanf("%" SCNu32 " %" SCNd32, &n, &pct) != 2) return 2;
      std::printf("%u\n", bs::sample_size(n, pct));
    } else if (!std::strcmp(cmd, "walk")) {
      uint32_t s0, N;
      if (std::scanf("%" SCNu32 " %" SCNu32, &s0, &N) != 2 || N == 0) return 2;
      const uint32_t s = bs::sample_start(s0, N), k1 = bs::sample_node(s, N > 1 ? 1 : 0, N);
      std::printf("%u %u %u %u %u\n", bs::sample_node(s, 0, N), k1, bs::sample_node(s, N - 1, N), bs::sample_pos(s, k1, N), bs::sample_step(s, N, N));
    } else if (!std::strcmp(cmd, "bit")) {
      uint64_t mask; uint32_t r;
      if (std::scanf("%" SCNx64 " %" SCNu32, &mask, &r) != 2) return 2;
      std::printf("%u\n", bs::sample_nth_bit(mask, r));
    } else return 2;
  }
  return failures ? 1 : 0;
}
