// Stand-alone driver of nom_own_check (csrc/bs_nominated_check.hpp; tests/test_seq_nominated_cpu.py builds it under ASan + UBSan): what
// bs_seq_run_nominated refuses about its own_id array, and the translation of ids to row indices.  One case per line, one answer line per
// case.  Arrays hold exactly the counts (a read past one is a sanitizer report); has_own 0 passes NULL.
//   w live[w] ids p has_own own[p if has_own]   ->   "code" and, on 0, " row[p]"
#include <cstdio>
#include <vector>

#include "bs_nominated_check.hpp"

int main() {
  unsigned w;
  while (std::scanf("%u", &w) == 1) {
    std::vector<uint32_t> live(w);
    for (auto& x : live)
      if (std::scanf("%u", &x) != 1) return 2;
    unsigned ids, p, has_own;
    if (std::scanf("%u %u %u", &ids, &p, &has_own) != 3) return 2;
    std::vector<uint32_t> own(has_own ? p : 0);
    for (auto& x : own)
      if (std::scanf("%u", &x) != 1) return 2;
    std::vector<uint32_t> rows{12345u};                      // (left untouched on a refusal)
    const int code = bs::nom_own_check(live.empty() ? nullptr : live.data(), w, ids, p, has_own ? (own.empty() ? live.data() : own.data()) : nullptr,
                                       0xFFFFFFFFu, rows);
    std::printf("%d", code);
    if (code == bs::kNomOk) {
      if (rows.size() != p) return 3;
      for (uint32_t r : rows) std::printf(" %u", r);
    } else if (rows.size() != 1 || rows[0] != 12345u || !bs::nom_own_check_text(code)[0]) {
      return 3;
    }
    std::printf("\n");
  }
  return 0;
}
