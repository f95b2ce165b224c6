// Stand-alone driver of csrc/bs_nominated_nodes_check.hpp (tests/test_nominated_nodes_cpu.py builds it under ASan + UBSan).  One case per
// line, one answer line per case.  Arrays hold exactly the counts (a read past one is a sanitizer report); a `null` flag passes NULL instead.
//   C n0 n_now w count null_list kind[count] index[count] cap null_out null_n
//        nom_nodes_check -> "code"; on 0 also " n_new appended moves R removed[R]" (moves: nom_nodes_moves for a table of w rows)
//   L w live[w] n gone[n]
//        nom_nodes_live_drop -> "left[..]" (the count first)
#include <cstdio>
#include <vector>

#include "bs_nominated_nodes_check.hpp"

static bool read_list(std::vector<uint32_t>& v) {
  for (auto& x : v)
    if (std::scanf("%u", &x) != 1) return false;
  return true;
}

int main() {
  char what[4];
  while (std::scanf("%3s", what) == 1) {
    if (what[0] == 'C') {
      unsigned n0, n_now, w, count, null_list, cap, null_out, null_n;
      if (std::scanf("%u %u %u %u %u", &n0, &n_now, &w, &count, &null_list) != 5) return 2;
      std::vector<uint32_t> kind(null_list ? 0 : count), index(null_list ? 0 : count);
      if (!read_list(kind) || !read_list(index) || std::scanf("%u %u %u", &cap, &null_out, &null_n) != 3) return 2;
      std::vector<uint32_t> id(null_out ? 0 : cap), node(null_out ? 0 : cap);
      std::vector<int32_t> prio(null_out ? 0 : cap);
      uint32_t n = 77;
      bs::NodeReplay rp;
      const int code = bs::nom_nodes_check(n0, n_now, count, kind.empty() ? nullptr : kind.data(), index.empty() ? nullptr : index.data(), cap,
                                           id.empty() ? nullptr : id.data(), node.empty() ? nullptr : node.data(),
                                           prio.empty() ? nullptr : prio.data(), null_n ? nullptr : &n, rp);
      std::printf("%d", code);
      if (code == bs::kNomNodesOk) {
        std::printf(" %u %u %d %zu", rp.n_new, rp.appended, bs::nom_nodes_moves(w, n0, rp) ? 1 : 0, rp.removed.size());
        for (uint32_t r : rp.removed) std::printf(" %u", r);
      }
      std::printf("\n");
      if (n != 77) return 3;                                // (the check writes no output)
    } else if (what[0] == 'L') {
      unsigned w, n;
      if (std::scanf("%u", &w) != 1) return 2;
      std::vector<uint32_t> live(w);
      if (!read_list(live) || std::scanf("%u", &n) != 1) return 2;
      std::vector<uint32_t> gone(n);
      if (!read_list(gone)) return 2;
      bs::nom_nodes_live_drop(live, gone.empty() ? nullptr : gone.data(), gone.size());
      std::printf("%zu", live.size());
      for (uint32_t x : live) std::printf(" %u", x);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  std::printf("%s\n", bs::nom_nodes_check_text(bs::kNomNodesOk));
  return 0;
}
