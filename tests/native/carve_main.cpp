// Stand-alone driver of csrc/bs_carve.hpp (tests/test_carve_cpu.py compiles it under ASan + UBSan and reads its output).
// For pad 256 and pad 1 and every rotation of the counts it carves eight pieces of mixed element types, prints
//   P <pad> <run> <sizeof T> <n> <off> <bytes()>      one line per piece
//   T <pad> <run> <mark()>                            the total
// and stores the first and the last element of every piece into a heap block of exactly mark() bytes: a piece that reaches past the
// total, or past its successor's start, is a heap overflow for ASan.  A packed run (pad 1) takes its 8-byte columns first, as the one
// packed layout of the library does, so that every store is aligned.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "bs_carve.hpp"

struct Rec { int64_t a; uint32_t b, c; int64_t d; };
static_assert(sizeof(Rec) == 24, "the 24-byte element");

static const size_t kCounts[7] = {0, 1, 63, 64, 65, 257, 1000};

template <class T>
static bs::Piece<T> piece(bs::Carve& cv, size_t n, size_t pad, int run, std::vector<std::pair<size_t, size_t>>& spans) {
  const bs::Piece<T> p = cv.take<T>(n, pad);
  std::printf("P %zu %d %zu %zu %zu %zu\n", pad, run, sizeof(T), p.n, p.off, p.bytes());
  spans.push_back({p.off, p.bytes()});
  return p;
}

template <class T>
static void touch(const bs::Piece<T>& p, uint8_t* base, uint8_t tag) {
  if (!p.n) return;
  T first, last;
  std::memset(&first, tag, sizeof(T));
  std::memset(&last, tag ^ 0xFF, sizeof(T));
  p.in(base)[p.n - 1] = last;
  p.in(base)[0] = first;
  const uint8_t* cb = base;
  const T* r = p.in(cb);                                  // the const form names the same bytes
  if (std::memcmp(&r[0], &first, sizeof(T)) || (p.n > 1 && std::memcmp(&r[p.n - 1], &last, sizeof(T)))) { std::printf("FAIL readback\n"); std::exit(1); }
}

static void run(size_t pad, int r) {
  const size_t* k = kCounts;
  auto n = [&](int i) { return k[(r + i) % 7]; };
  bs::Carve cv;
  if (cv.mark() != 0) { std::printf("FAIL a carve starts at 0\n"); std::exit(1); }
  std::vector<std::pair<size_t, size_t>> spans;
  // pad 256: the types in mixed order; pad 1: the same eight pieces, 8-byte elements first
  const bool packed = pad == 1;
  bs::Piece<uint8_t> a, f;
  bs::Piece<uint32_t> b, e;
  bs::Piece<int64_t> c, h;
  bs::Piece<Rec> d, g;
  if (!packed) {
    a = piece<uint8_t>(cv, n(0), pad, r, spans);
    b = piece<uint32_t>(cv, n(1), pad, r, spans);
    c = piece<int64_t>(cv, n(2), pad, r, spans);
    d = piece<Rec>(cv, n(3), pad, r, spans);
    e = piece<uint32_t>(cv, n(4), pad, r, spans);
    f = piece<uint8_t>(cv, n(5), pad, r, spans);
    g = piece<Rec>(cv, n(6), pad, r, spans);
    h = piece<int64_t>(cv, n(7), pad, r, spans);
  } else {
    c = piece<int64_t>(cv, n(2), pad, r, spans);
    d = piece<Rec>(cv, n(3), pad, r, spans);
    g = piece<Rec>(cv, n(6), pad, r, spans);
    h = piece<int64_t>(cv, n(7), pad, r, spans);
    b = piece<uint32_t>(cv, n(1), pad, r, spans);
    e = piece<uint32_t>(cv, n(4), pad, r, spans);
    a = piece<uint8_t>(cv, n(0), pad, r, spans);
    f = piece<uint8_t>(cv, n(5), pad, r, spans);
  }
  const size_t total = cv.mark();
  std::printf("T %zu %d %zu\n", pad, r, total);
  for (size_t i = 0; i < spans.size(); ++i) {              // inside the total, and no piece reaches into the next one
    const size_t end = spans[i].first + spans[i].second;
    if (end > total || (i + 1 < spans.size() && end > spans[i + 1].first)) { std::printf("FAIL overlap\n"); std::exit(1); }
  }
  uint8_t* buf = new uint8_t[total];                       // exactly mark() bytes
  touch(a, buf, 1); touch(b, buf, 2); touch(c, buf, 3); touch(d, buf, 4);
  touch(e, buf, 5); touch(f, buf, 6); touch(g, buf, 7); touch(h, buf, 8);
  delete[] buf;
}

int main() {
  const bs::Piece<int64_t> p{512, 4};
  void* none = nullptr;
  const void* cnone = nullptr;
  if (p.in(none) != nullptr || p.in(cnone) != nullptr) { std::printf("FAIL in(nullptr) is not null\n"); return 1; }
  for (size_t pad : {(size_t)256, (size_t)1})
    for (int r = 0; r < 7; ++r) run(pad, r);
  std::printf("OK\n");
  return 0;
}
