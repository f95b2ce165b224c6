// bs_carve.hpp — how the host lays several arrays out in one allocation (a staging vector, a device scratch block, a read-back
// block): a running offset hands out typed pieces, and a piece knows its element type, so the width of an array is written once,
// in take<T>(n), and not again at the pointer cast and at every copy.  Plain C++17, no HIP header: tests/native/carve_main.cpp
// compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bs {

// n elements of T at byte offset `off` of some base
template <class T>
struct Piece {
  size_t off = 0, n = 0;
  size_t bytes() const { return n * sizeof(T); }
  // null for a base that does not exist yet (null + n is undefined behaviour even if nobody follows the pointer)
  T* in(void* base) const { return base ? reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off) : nullptr; }
  const T* in(const void* base) const { return base ? reinterpret_cast<const T*>(static_cast<const uint8_t*>(base) + off) : nullptr; }
};

// The running offset.  take<T>(n) is the piece at the current offset; the next one starts at its end rounded up to `pad` (256: what
// the device pieces are aligned to; 1: packed).  An empty piece takes no bytes.  mark() is the current offset: a boundary or the total.
class Carve {
  size_t o_ = 0;

 public:
  template <class T>
  Piece<T> take(size_t n, size_t pad = 256) {
    const Piece<T> p{o_, n};
    o_ = (o_ + p.bytes() + pad - 1) / pad * pad;
    return p;
  }
  size_t mark() const { return o_; }
};

}  // namespace bs
