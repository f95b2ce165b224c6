// Stand-alone driver of csrc/bs_nominated_check.hpp (tests/test_nominated_cpu.py builds it under ASan + UBSan).  One case per line -> the
// check's code.  Arrays hold exactly the counts (a read past one is a sanitizer report); a `null` flag passes NULL instead.
//   D n m null max_rows node[m]                                          nom_load_check (the four columns share the flag; m above
//                                                                        max_rows sends no node list: the check must not walk it)
//   A w ids live[w] nr null_r rem[nr] ni null_i pod[ni] node[ni] p n max_rows max_ids     nom_apply_check
//   N w ids count max_rows max_ids                                       nom_nominate_check
#include <cstdio>
#include <vector>

#include "bs_nominated_check.hpp"

static bool read_list(std::vector<uint32_t>& v) {
  for (auto& x : v)
    if (std::scanf("%u", &x) != 1) return false;
  return true;
}

int main() {
  char kind[4];
  while (std::scanf("%3s", kind) == 1) {
    if (kind[0] == 'D') {
      unsigned n, m, null, max_rows;
      if (std::scanf("%u %u %u %u", &n, &m, &null, &max_rows) != 4) return 2;
      const bool listed = m <= max_rows;
      std::vector<uint32_t> node(listed ? m : 0), pres(listed ? m : 0);
      std::vector<int32_t> prio(listed ? m : 0);
      std::vector<int64_t> req(listed ? m : 0);
      if (!read_list(node)) return 2;
      const bool z = null || !listed || m == 0;             // (an empty vector's data() may be anything: pass NULL)
      std::printf("%d\n", bs::nom_load_check(n, m, z ? nullptr : node.data(), z ? nullptr : prio.data(), z ? nullptr : req.data(),
                                             z ? nullptr : pres.data(), max_rows));
    } else if (kind[0] == 'A') {
      unsigned w, ids, nr, null_r, ni, null_i, p, n, max_rows, max_ids;
      if (std::scanf("%u %u", &w, &ids) != 2) return 2;
      std::vector<uint32_t> live(w);
      if (!read_list(live) || std::scanf("%u %u", &nr, &null_r) != 2) return 2;
      std::vector<uint32_t> rem(null_r ? 0 : nr);
      if (!read_list(rem) || std::scanf("%u %u", &ni, &null_i) != 2) return 2;
      std::vector<uint32_t> pod(null_i ? 0 : ni), node(null_i ? 0 : ni);
      std::vector<int32_t> prio(null_i ? 0 : ni);
      if (!read_list(pod) || !read_list(node) || std::scanf("%u %u %u %u", &p, &n, &max_rows, &max_ids) != 4) return 2;
      std::printf("%d\n", bs::nom_apply_check(w ? live.data() : nullptr, w, ids, nr, rem.empty() ? nullptr : rem.data(), ni,
                                              pod.empty() ? nullptr : pod.data(), node.empty() ? nullptr : node.data(),
                                              prio.empty() ? nullptr : prio.data(), p, n, max_rows, max_ids));
    } else if (kind[0] == 'N') {
      unsigned w, ids, count, max_rows, max_ids;
      if (std::scanf("%u %u %u %u %u", &w, &ids, &count, &max_rows, &max_ids) != 5) return 2;
      std::printf("%d\n", bs::nom_nominate_check(w, ids, count, max_rows, max_ids));
    } else {
      return 2;
    }
  }
  std::printf("%s\n", bs::nom_check_text(bs::kNomOk));
  return 0;
}
