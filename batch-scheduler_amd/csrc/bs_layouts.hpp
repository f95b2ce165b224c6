// bs_layouts.hpp — the layouts of the packs the context keeps in ONE allocation each (pods, groups, results): which typed pieces, in which
// order, for how many elements.  A layout is a value: bs_ctx holds the ones of its resident packs, a call that stages or gathers a pack
// carves its own.  Plain C++17, no HIP header: tests/native/layouts_main.cpp compiles it alone.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "bs_carve.hpp"

namespace bs {

// One pod pack = the arrays of bs_pods_soa for exactly `p` pods (the part a load uploads in ONE copy, `in_bytes`) followed by
// the per-pod ids the library derives (request class, (group, class) pair): what travels with a pod when the queue is patched.
// The pinned staging buffer uses the same layout (input part only) — and its OWN copy of it (bs_pods_map must not disturb the
// resident queue).
struct PodLayout {
  Piece<int32_t> group;
  Piece<int64_t> req;
  Piece<uint32_t> pres, cls, pclass, ppair;
  Piece<uint64_t> owner;
  Piece<uint8_t> flags;
  size_t in_bytes = 0, bytes = 0;
  uint32_t p = 0;
};
inline PodLayout pod_layout(uint32_t P, uint32_t L) {
  const size_t n = std::max<uint32_t>(P, 1);
  PodLayout l;
  Carve cv;
  l.group = cv.take<int32_t>(n);
  l.req = cv.take<int64_t>(n * L);
  l.pres = cv.take<uint32_t>(n);
  l.cls = cv.take<uint32_t>(n);
  l.owner = cv.take<uint64_t>(n);
  l.flags = cv.take<uint8_t>(n);
  l.in_bytes = cv.mark();
  l.pclass = cv.take<uint32_t>(n);
  l.ppair = cv.take<uint32_t>(n);
  l.bytes = cv.mark();
  l.p = P;
  return l;
}

// One group pack = the arrays of bs_groups_soa for exactly `g` groups in one allocation (the live pack, the twin bs_groups_list_apply gathers
// into, and that call's rows in pinned memory): carved in this order wherever a pack is laid out.  `bytes` is the running offset behind the
// last piece: the pack's size where the carve started at 0.
struct GroupLayout {
  Piece<uint32_t> mm, sc, matched, cls, mrpres;
  Piece<uint8_t> flags;
  Piece<int64_t> minres;
  Piece<uint64_t> occ;
  size_t bytes = 0;
  uint32_t g = 0;
};
inline GroupLayout group_carve(Carve& cv, uint32_t G, uint32_t L) {
  const size_t n = std::max<uint32_t>(G, 1);
  GroupLayout l;
  l.mm = cv.take<uint32_t>(n);
  l.sc = cv.take<uint32_t>(n);
  l.matched = cv.take<uint32_t>(n);
  l.flags = cv.take<uint8_t>(n);
  l.cls = cv.take<uint32_t>(n);
  l.minres = cv.take<int64_t>(n * L);
  l.mrpres = cv.take<uint32_t>(n);
  l.occ = cv.take<uint64_t>(n);
  l.bytes = cv.mark();
  l.g = G;
  return l;
}

// The result pack = everything bs_batch_read returns in its first copy: the per-pod arrays | admit[G] | ready[G].
struct OutLayout {
  Piece<uint8_t> pf_code, fl_code, ready;
  Piece<uint32_t> pf_first_k, fl_feasible, fl_slot, admit;
  Piece<int32_t> pf_leader;
  size_t bytes = 0;
};
inline OutLayout out_layout(uint32_t P, uint32_t G) {
  const size_t n = std::max<uint32_t>(P, 1), g = std::max<uint32_t>(G, 1);
  OutLayout l;
  Carve cv;
  l.pf_code = cv.take<uint8_t>(n);
  l.pf_first_k = cv.take<uint32_t>(n);
  l.pf_leader = cv.take<int32_t>(n);
  l.fl_code = cv.take<uint8_t>(n);
  l.fl_feasible = cv.take<uint32_t>(n);
  l.fl_slot = cv.take<uint32_t>(n);
  l.admit = cv.take<uint32_t>(g);
  l.ready = cv.take<uint8_t>(g);
  l.bytes = cv.mark();
  return l;
}

}  // namespace bs
