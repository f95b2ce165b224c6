// Stand-alone driver of csrc/bs_wait_list.hpp (tests/test_wait_cpu.py builds it under ASan + UBSan).  One case per line -> the check's code.
//   L bound null count list[count]      wait_list_check (groups: bound = g; ids: bound = the id space)
//   B bound count a b c d               the same with only the four entries given and `count` passed as it stands (a count far above the
//                                       bound must be answered without touching more of the list)
//   F flags                             wait_flags_check
//   W n g null w node[w] group[w]       wait_load_check
#include <cstdio>
#include <vector>

#include "bs_wait_list.hpp"

int main() {
  char kind[4];
  while (std::scanf("%3s", kind) == 1) {
    if (kind[0] == 'F') {
      unsigned flags;
      if (std::scanf("%u", &flags) != 1) return 2;
      std::printf("%d\n", bs::wait_flags_check(flags));
    } else if (kind[0] == 'B') {
      unsigned bound, count;
      std::vector<uint32_t> four(4);
      if (std::scanf("%u %u %u %u %u %u", &bound, &count, &four[0], &four[1], &four[2], &four[3]) != 6) return 2;
      std::printf("%d\n", bs::wait_list_check(bound, count, four.data()));
    } else if (kind[0] == 'L') {
      unsigned bound, null, count;
      if (std::scanf("%u %u %u", &bound, &null, &count) != 3) return 2;
      std::vector<uint32_t> list(count);                      // exactly `count` elements: a read past the list is a sanitizer report
      for (unsigned i = 0; i < count; ++i)
        if (std::scanf("%u", &list[i]) != 1) return 2;
      static uint32_t none;
      const uint32_t* p = null ? nullptr : (count ? list.data() : &none);
      std::printf("%d\n", bs::wait_list_check(bound, count, p));
    } else if (kind[0] == 'W') {
      unsigned n, g, null, w;
      if (std::scanf("%u %u %u %u", &n, &g, &null, &w) != 4) return 2;
      std::vector<uint32_t> node(w);
      std::vector<int32_t> group(w);
      for (unsigned i = 0; i < w; ++i)
        if (std::scanf("%u", &node[i]) != 1) return 2;
      for (unsigned i = 0; i < w; ++i)
        if (std::scanf("%d", &group[i]) != 1) return 2;
      static uint32_t none_u;
      static int32_t none_i;
      std::printf("%d\n", bs::wait_load_check(n, g, w, null ? nullptr : (w ? node.data() : &none_u), null ? nullptr : (w ? group.data() : &none_i)));
    } else {
      return 2;
    }
  }
  return 0;
}
