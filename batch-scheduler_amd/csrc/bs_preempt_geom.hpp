// Launch geometry of the preemption search (bs_preempt_run, bs_preempt_commit; tu_preempt.hip): how the node list is cut into chunks for the
// grid (slot tiles, node chunks).  Plain C++ arithmetic, no HIP includes: the CPU tests compile it on its own
// (tests/test_preempt_geom_cpu.py).  Both entry points call preempt_geom(); nobody restates the arithmetic.
//
//   tiles       = preempt_tiles(count) = cdiv(count, 64)     64 slots a wave, one wave a block
//   nchunks     about kPreemptWaves / tiles blocks along y, at most one per node, at least one
//   chunk_nodes = cdiv(N, nchunks) nodes a chunk; nchunks is then cut back to cdiv(N, chunk_nodes), so the chunks cover [0, N) with
//                 none empty: (nchunks - 1) * chunk_nodes < N <= nchunks * chunk_nodes for N > 0
//
// The shipped numbers keep bs_preempt_commit's rescan list (k_pc_resolve's s_res, pc_threads<S>() entries) from ever filling: a slot
// lists a chunk only when kPcK = 4 recorded nodes of it are dirty, so T + 1 listed chunks need 4 (T + 1) dirty nodes, and a call has
// at most count <= 64 tiles nominees.  For T = 512 and T = 256: nchunks <= T or 4 (T + 1) > 64 tiles.  The list's spill path is live code
// all the same; the test hook below reaches it (tests/test_gpu_preempt_commit_chunks.py), and the CPU test asserts the inequality, so
// whoever retunes kPreemptWaves learns that the spill became reachable in production.
//
// forced_chunk_nodes (BS_TEST_PC_CHUNK_NODES, a test hook read at context creation): a positive value sets chunk_nodes, clamped to
// [1, max(N, 1)], and nchunks follows as cdiv(N, chunk_nodes).  0 is the shipped geometry.  A forced value whose nchunks would exceed
// the grid's y limit is ignored for that call.
#pragma once
#include <cstdint>

namespace bs {

constexpr uint32_t kPreemptWaves = 4096;        // waves in the first launch: 16 per CU
constexpr uint32_t kPreemptGridYMax = 65535;    // blocks along y

struct PreemptGeom {
  uint32_t tiles, nchunks, chunk_nodes;
};

constexpr uint32_t preempt_cdiv(uint32_t a, uint32_t b) { return (a + b - 1u) / b; }
constexpr uint32_t preempt_tiles(uint32_t count) { return preempt_cdiv(count, 64u); }

// tiles >= 1 (the entry points return before the geometry for an empty call)
constexpr PreemptGeom preempt_geom_tiles(uint32_t n_nodes, uint32_t tiles, uint32_t forced_chunk_nodes = 0) {
  const uint32_t n1 = n_nodes > 1u ? n_nodes : 1u;
  if (forced_chunk_nodes) {
    const uint32_t cn = forced_chunk_nodes < n1 ? forced_chunk_nodes : n1;
    const uint32_t nch = preempt_cdiv(n_nodes, cn) > 1u ? preempt_cdiv(n_nodes, cn) : 1u;
    if (nch <= kPreemptGridYMax) return PreemptGeom{tiles, nch, cn};
  }
  // node chunks: about kPreemptWaves waves in the first launch, at least one node per chunk
  const uint32_t want = preempt_cdiv(kPreemptWaves, tiles);
  uint32_t nchunks = n1 < want ? n1 : want;
  if (nchunks < 1u) nchunks = 1u;
  uint32_t chunk_nodes = preempt_cdiv(n_nodes, nchunks);
  if (chunk_nodes < 1u) chunk_nodes = 1u;
  nchunks = preempt_cdiv(n_nodes, chunk_nodes);
  if (nchunks < 1u) nchunks = 1u;
  return PreemptGeom{tiles, nchunks, chunk_nodes};
}

constexpr PreemptGeom preempt_geom(uint32_t n_nodes, uint32_t count, uint32_t forced_chunk_nodes = 0) {
  return preempt_geom_tiles(n_nodes, preempt_tiles(count), forced_chunk_nodes);
}

}  // namespace bs
