// Stand-alone driver of csrc/bs_bound_bind_check.hpp (tests/test_bound_bind_cpu.py builds it under ASan + UBSan).  One case per line -> the
// check's code.
//   A nw null_w np null_p null_prio null_start          bind_args_check (arrays of exactly the counts, or NULL)
//   L wait_ids wait_rows nw id[nw] queue np pod[np]     bind_lists_check (lists of exactly the counts: a read past one is a sanitizer report)
//   I ids nw np limit                                   bind_ids_check
#include <cstdio>
#include <vector>

#include "bs_bound_bind_check.hpp"

int main() {
  char kind[4];
  while (std::scanf("%3s", kind) == 1) {
    if (kind[0] == 'A') {
      unsigned nw, zw, np, zp, zprio, zstart;
      if (std::scanf("%u %u %u %u %u %u", &nw, &zw, &np, &zp, &zprio, &zstart) != 6) return 2;
      std::vector<uint32_t> w(nw), p(np);
      std::vector<int32_t> prio(nw + np);
      std::vector<int64_t> start(nw + np);
      static uint32_t none_u;
      static int32_t none_i;
      static int64_t none_l;
      std::printf("%d\n", bs::bind_args_check(nw, zw ? nullptr : (nw ? w.data() : &none_u), np, zp ? nullptr : (np ? p.data() : &none_u),
                                              zprio ? nullptr : (nw + np ? prio.data() : &none_i), zstart ? nullptr : (nw + np ? start.data() : &none_l)));
    } else if (kind[0] == 'L') {
      unsigned ids, rows, nw, queue, np;
      if (std::scanf("%u %u %u", &ids, &rows, &nw) != 3) return 2;
      std::vector<uint32_t> w(nw);
      for (unsigned i = 0; i < nw; ++i)
        if (std::scanf("%u", &w[i]) != 1) return 2;
      if (std::scanf("%u %u", &queue, &np) != 2) return 2;
      std::vector<uint32_t> p(np);
      for (unsigned i = 0; i < np; ++i)
        if (std::scanf("%u", &p[i]) != 1) return 2;
      static uint32_t none;
      std::printf("%d\n", bs::bind_lists_check(ids, rows, nw, nw ? w.data() : &none, queue, np, np ? p.data() : &none));
    } else if (kind[0] == 'I') {
      unsigned ids, nw, np, limit;
      if (std::scanf("%u %u %u %u", &ids, &nw, &np, &limit) != 4) return 2;
      const int code = bs::bind_ids_check(ids, nw, np, limit);
      if (!bs::bind_check_text(code)[0]) return 3;
      std::printf("%d\n", code);
    } else {
      return 2;
    }
  }
  return 0;
}
