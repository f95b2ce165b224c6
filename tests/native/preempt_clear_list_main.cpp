// Stand-alone driver of csrc/bs_preempt_clear_list.hpp (tests/test_preempt_clear_cpu.py builds it under ASan + UBSan).  One case per
// line -> the check's code, and for R the rows that came back.  Arrays hold exactly the counts (a read or write past one is a sanitizer
// report); a `null` flag passes NULL instead.
//   C w live[w] n q count null id[count] node[count] by[count]           clear_list_check
//   R have m id[m] node[m] prio[m] by[m] cap null null_n                 clear_read -> code n_out id.. node.. prio.. by.. (min(m, cap) each)
#include <cstdio>
#include <vector>

#include "bs_preempt_clear_list.hpp"

static bool read_list(std::vector<uint32_t>& v) {
  for (auto& x : v)
    if (std::scanf("%u", &x) != 1) return false;
  return true;
}

int main() {
  char kind[4];
  while (std::scanf("%3s", kind) == 1) {
    if (kind[0] == 'C') {
      unsigned w, n, q, count, null;
      if (std::scanf("%u", &w) != 1) return 2;
      std::vector<uint32_t> live(w);
      if (!read_list(live) || std::scanf("%u %u %u %u", &n, &q, &count, &null) != 4) return 2;
      std::vector<uint32_t> id(null ? 0 : count), node(null ? 0 : count), by(null ? 0 : count);
      if (!read_list(id) || !read_list(node) || !read_list(by)) return 2;
      const bool z = id.empty();                            // (an empty vector's data() may be anything: pass NULL)
      std::printf("%d\n", bs::clear_list_check(count, z ? nullptr : id.data(), z ? nullptr : node.data(), z ? nullptr : by.data(),
                                               w ? live.data() : nullptr, w, n, q));
    } else if (kind[0] == 'R') {
      unsigned have, m, cap, null, null_n;
      if (std::scanf("%u %u", &have, &m) != 2) return 2;
      bs::ClearedRows rows;
      rows.reset(have != 0);
      rows.id.resize(m); rows.node.resize(m); rows.by.resize(m);
      std::vector<uint32_t> prio(m);
      if (!read_list(rows.id) || !read_list(rows.node) || !read_list(prio) || !read_list(rows.by)) return 2;
      rows.priority.assign(prio.begin(), prio.end());
      if (std::scanf("%u %u %u", &cap, &null, &null_n) != 3) return 2;
      const bool z = null || cap == 0;
      std::vector<uint32_t> id(z ? 0 : cap), node(z ? 0 : cap), by(z ? 0 : cap);
      std::vector<int32_t> pr(z ? 0 : cap);
      uint32_t n_out = 0xDEADu;
      const int code = bs::clear_read(rows, cap, z ? nullptr : id.data(), z ? nullptr : node.data(), z ? nullptr : pr.data(),
                                      z ? nullptr : by.data(), null_n ? nullptr : &n_out);
      std::printf("%d %u", code, n_out);
      const size_t k = code == bs::kClrOk && !z ? (m < cap ? m : cap) : 0;
      for (size_t i = 0; i < k; ++i) std::printf(" %u", id[i]);
      for (size_t i = 0; i < k; ++i) std::printf(" %u", node[i]);
      for (size_t i = 0; i < k; ++i) std::printf(" %d", pr[i]);
      for (size_t i = 0; i < k; ++i) std::printf(" %u", by[i]);
      std::printf("\n");
    } else {
      return 2;
    }
  }
  std::printf("%s\n", bs::clear_check_text(bs::kClrOk));
  return 0;
}
