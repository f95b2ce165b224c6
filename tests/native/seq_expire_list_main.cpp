// Stand-alone driver of csrc/bs_seq_expire_list.hpp (tests/test_seq_expire_cpu.py builds it under ASan + UBSan).
// One case per line: g flags null count list[count]  ->  the check's code, one per line.  "g flags null count big a b c d": the list is
// only the four entries given, `count` is passed as it stands (a count far above g must be answered without touching more of the list).
#include <cstdio>
#include <vector>

#include "bs_seq_expire_list.hpp"

int main() {
  unsigned g, flags, null, count;
  while (std::scanf("%u %u %u %u", &g, &flags, &null, &count) == 4) {
    char word[8];
    if (count > 1000000u) {
      std::vector<uint32_t> four(4);
      if (std::scanf("%7s %u %u %u %u", word, &four[0], &four[1], &four[2], &four[3]) != 5) return 2;
      std::printf("%d\n", bs::seq_expire_list_check(g, count, four.data(), flags));
      continue;
    }
    std::vector<uint32_t> list(count + 1u);                   // (never a NULL pointer for an empty list)
    for (unsigned i = 0; i < count; ++i)
      if (std::scanf("%u", &list[i]) != 1) return 2;
    list.resize(count);
    list.shrink_to_fit();                                     // exactly `count` elements: a read past the list is a sanitizer report
    std::vector<uint32_t> exact(list.begin(), list.end());
    static uint32_t none;
    const uint32_t* p = null ? nullptr : (count ? exact.data() : &none);
    std::printf("%d\n", bs::seq_expire_list_check(g, count, p, flags));
  }
  return 0;
}
