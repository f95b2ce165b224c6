// bs_bound_cols.hpp — the bound-pod table's columns as the host names them: what tu_bound.hip (the table's own calls) and tu_preempt.hip (the
// victim search and the plans, which read the table and compact it) share.  Host code only: no kernel, and no HIP header beyond what
// bs_kernels.hpp brings for BoundLayout.
#pragma once
#include <type_traits>

#include "bs_carve.hpp"
#include "bs_kernels.hpp"

namespace bs {

// The bound-pod table: its nine columns at the offsets of a BoundLayout (bound_layout, bs_kernels.hpp), typed once.  U8 is
// uint8_t (a table that is written: the staging copy of a load, a compaction target) or const uint8_t; a null base gives null columns.
template <class U8>
struct BoundCols {
  template <class T> using Col = std::conditional_t<std::is_const_v<U8>, const T, T>*;
  Col<uint32_t> boff, id, pres, nviol;
  Col<int32_t> prio, group;
  Col<int64_t> start, req;
  Col<uint8_t> pdb;
};
template <class U8>
BoundCols<U8> bound_cols(U8* base, const BoundLayout& l) {
  return {Piece<uint32_t>{l.boff}.in(base), Piece<uint32_t>{l.id}.in(base), Piece<uint32_t>{l.pres}.in(base), Piece<uint32_t>{l.nviol}.in(base), Piece<int32_t>{l.prio}.in(base),
          Piece<int32_t>{l.group}.in(base), Piece<int64_t>{l.start}.in(base), Piece<int64_t>{l.req}.in(base), Piece<uint8_t>{l.pdb}.in(base)};
}
// the seven columns every device struct over the table names (PreemptDev, CommitDev, CompactDev, BoundApplyDev, BoundNodesDev); bpres and
// bnviol are set from the returned view where the struct has them
template <class D, class U8>
BoundCols<U8> bound_dev(D& d, U8* base, const BoundLayout& l) {
  const BoundCols<U8> t = bound_cols(base, l);
  d.boff = t.boff; d.bprio = t.prio; d.bstart = t.start; d.bgroup = t.group; d.bid = t.id; d.breq = t.req; d.bpdb = t.pdb;
  return t;
}

}  // namespace bs
