// Stand-alone driver of csrc/bs_layouts.hpp (tests/test_layouts_cpu.py compiles it under ASan + UBSan and reads its output).
// For P and G in {0, 1, 63, 64, 65, 257} and L in {1, 4, 8} it prints the three pack layouts:
//   C <pack> <a> <b> <column> <off> <n> <i|u><sizeof T>    one line per piece (i: a signed element type), in the order the carve takes them
//   T <pack> <a> <b> <name> <value>                   the totals and the counts a layout carries
// where <pack> <a> <b> is `pod P L`, `group G L` (group_carve from offset 0) or `out P G`.  Every piece's first and last element
// is stored into a heap block of exactly `bytes` bytes: a piece that reaches past the total is a heap overflow for ASan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "bs_layouts.hpp"

static const uint32_t kSizes[6] = {0, 1, 63, 64, 65, 257};
static const uint32_t kLanes[3] = {1, 4, 8};

struct Out {
  const char* pack;
  uint32_t a, b;
  uint8_t* buf;
  template <class T>
  void col(const char* name, const bs::Piece<T>& p) const {
    std::printf("C %s %u %u %s %zu %zu %c%zu\n", pack, a, b, name, p.off, p.n, std::is_signed<T>::value ? 'i' : 'u', sizeof(T));
    T v;
    std::memset(&v, 0x5A, sizeof(T));
    p.in(buf)[0] = v;
    p.in(buf)[p.n - 1] = v;
  }
  void total(const char* name, size_t v) const { std::printf("T %s %u %u %s %zu\n", pack, a, b, name, v); }
};

int main() {
  for (uint32_t L : kLanes)
    for (uint32_t n : kSizes) {
      const bs::PodLayout p = bs::pod_layout(n, L);
      uint8_t* pb = new uint8_t[p.bytes];
      const Out po{"pod", n, L, pb};
      po.col("group", p.group); po.col("req", p.req); po.col("pres", p.pres); po.col("cls", p.cls); po.col("owner", p.owner); po.col("flags", p.flags);
      po.col("pclass", p.pclass); po.col("ppair", p.ppair);
      po.total("in_bytes", p.in_bytes); po.total("bytes", p.bytes); po.total("p", p.p);
      delete[] pb;

      bs::Carve cv;
      const bs::GroupLayout g = bs::group_carve(cv, n, L);
      uint8_t* gb = new uint8_t[g.bytes];
      const Out go{"group", n, L, gb};
      go.col("mm", g.mm); go.col("sc", g.sc); go.col("matched", g.matched); go.col("flags", g.flags); go.col("cls", g.cls); go.col("minres", g.minres);
      go.col("mrpres", g.mrpres); go.col("occ", g.occ);
      go.total("bytes", g.bytes); go.total("mark", cv.mark()); go.total("g", g.g);
      delete[] gb;
    }
  for (uint32_t P : kSizes)
    for (uint32_t G : kSizes) {
      const bs::OutLayout o = bs::out_layout(P, G);
      uint8_t* ob = new uint8_t[o.bytes];
      const Out oo{"out", P, G, ob};
      oo.col("pf_code", o.pf_code); oo.col("pf_first_k", o.pf_first_k); oo.col("pf_leader", o.pf_leader); oo.col("fl_code", o.fl_code);
      oo.col("fl_feasible", o.fl_feasible); oo.col("fl_slot", o.fl_slot); oo.col("admit", o.admit); oo.col("ready", o.ready);
      oo.total("bytes", o.bytes);
      delete[] ob;
    }
  std::printf("OK\n");
  return 0;
}
