// Stand-alone driver of csrc/bs_groups_list_check.hpp (tests/test_groups_list_cpu.py builds it under ASan + UBSan).  One case per line:
//   g null_mask n_remove remove[n_remove] n_update update[n_update] rows_g n_append wait_cap
// null_mask: 1 the remove list is NULL, 2 the update list, 4 a column of rows, 8 a result array.
// -> the check's code; for a valid delta also g_new, the new index of every old group, and groups_list_max_group(m) for m = -1 .. g.
#include <cstdio>
#include <vector>

#include "bs_groups_list_check.hpp"

int main() {
  unsigned g, mask, nr;
  while (std::scanf("%u %u %u", &g, &mask, &nr) == 3) {
    std::vector<uint32_t> rem(nr);                           // exactly as many elements as the count: a read past a list is a sanitizer report
    for (unsigned i = 0; i < nr; ++i)
      if (std::scanf("%u", &rem[i]) != 1) return 2;
    unsigned nu;
    if (std::scanf("%u", &nu) != 1) return 2;
    std::vector<uint32_t> upd(nu);
    for (unsigned i = 0; i < nu; ++i)
      if (std::scanf("%u", &upd[i]) != 1) return 2;
    unsigned rows_g, n_append, wait_cap;
    if (std::scanf("%u %u %u", &rows_g, &n_append, &wait_cap) != 3) return 2;
    static uint32_t none;
    const uint32_t* rp = (mask & 1u) ? nullptr : (nr ? rem.data() : &none);
    const uint32_t* up = (mask & 2u) ? nullptr : (nu ? upd.data() : &none);
    const int code = bs::groups_list_check(g, nr, rp, nu, up, rows_g, (mask & 4u) != 0, n_append, wait_cap, (mask & 8u) != 0);
    std::printf("%d", code);
    if (code == bs::kGlOk) {
      std::printf(" %u", bs::groups_list_count(g, nr, n_append));
      for (unsigned i = 0; i < g; ++i) std::printf(" %d", bs::groups_list_new_index(i, nr, rp));
      for (int m = -1; m <= (int)g; ++m) std::printf(" %d", bs::groups_list_max_group(m, g, nr, rp));
    }
    std::printf("\n");
  }
  return 0;
}
