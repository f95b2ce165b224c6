// Launch geometry of the steady-state chain (run_fast, bsched.hip): WHICH form of the step runs, the grid of every launch, and what the
// blocks of that grid add to the tickets.  Plain C++ arithmetic, no HIP includes: the CPU tests compile it on its own and walk it against a
// Python restatement (tests/test_step_geom_cpu.py, tests/step_geom_ref.py).  run_fast fills a StepIn, asks for a plan, launches what the plan
// says and advances the tickets by what the plan says; nobody restates the arithmetic.
//
// step_a_plan: the one-launch forms (k_fast_step_a; bs_ctx::step_a_form).  The grid is, in block order,
//
//   qb pod blocks | pb class-slot blocks | nchunks x nshares table blocks | fblocks Filter blocks        grid = the sum
//
// and the ticket advances are what those blocks add on the device (bs_fast.hpp, kTk*).  The two must agree: a block waits until a counter
// has moved by the number of its producers, so an advance that is not the number of blocks that add is a HANG, not a wrong answer.
//
//   kTkSlots (tk_pods)  += pb when there are class-slot blocks, qb otherwise     whoever publishes the class slots adds once
//   kTkTab   (tk_tab)   += nchunks unless whole                                  the first share of every table chunk (the whole-step form hands
//                                                                                the chunk totals over as tagged words: no ticket)
//   kTkP1    (tk_p1)    += qb when whole                                         the pod blocks' first halves
//   kTkDone  (tk_done)  += nchunks * nshares + fblocks when whole and qb > kGatherDirectBlocks   every table / Filter block of a large queue (a
//                                                                                small queue's producers leave tagged words, no counter)
//
// launch_b_plan: the legacy chain behind launch A (k_fast_query_tables) — one of five forms of launch B, then k_fast_final unless fused.
// The two residency comparisons (the occupancy API) stay with the caller: a plan exposes the grid, the caller asks the chip.
#pragma once
#include <cstdint>

#ifndef BS_GATHER_DIRECT
#define BS_GATHER_DIRECT 8
#endif

namespace bs {

constexpr int kTblChunk = 256;                 // rows per table chunk = threads per block of launch A and of k_fast_step_a
constexpr uint32_t kStepSlotsMax = 256;        // class slots the one-launch form handles (the latency regime: K <= 256)
constexpr uint32_t kGatherDirectBlocks = BS_GATHER_DIRECT;   // up to this many pod blocks poll the result words directly (fast_final_block<true>)

constexpr uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }   // host: grid sizes
constexpr uint32_t geom_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
constexpr uint32_t geom_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// The Filter role's block count: four waves a block, at most `waves`, one wave per (tile of 64 slots, two 64-node blocks).
constexpr uint32_t filter_blocks(uint32_t waves, uint32_t slot_tiles, uint32_t W) {
  return cdiv(geom_min(waves, slot_tiles * geom_max(1u, cdiv(W, 2u))), 4u);
}

struct StepIn {
  uint32_t P, G, N, M, S, W;                   // pods, groups, nodes, table rows, scalar lanes, cdiv(N, 64)
  // the class count and whether the host knows it: k_host = 0 while kinfo_pending, h_K (the last known K) otherwise
  uint32_t k_host, k_bound, h_K;
  bool kinfo_pending;
  uint32_t step_a_form, step_shares;
  bool step_a_on;
  uint32_t filter_waves;
  bool filter_waves_env;
  uint32_t tp_filter, tp_share, tp_fwaves, tp_tmin;
  uint32_t target_waves, scan_share;           // scan_share: the override (0 = none)
  uint32_t nranks;
  bool run_filter, dirs_ready;
  bool ranges_valid;                           // the gang-aligned pod ranges of the load still hold (and are on the device)
  uint32_t nranges;
  bool whole_bufs;                             // the record buffers of the whole-step form exist
  bool no_fuse_final, no_nodew, have_nodew;
  bool collect_stats;
  int enable_timing;
};

constexpr uint32_t table_chunks(uint32_t M) { return geom_max(1u, cdiv(M, 256u)); }

// The class count the one-launch forms size their grid for.  K not on the host yet (the queue was patched a moment ago and nobody has waited
// for the patch's word): the whole-step form takes a BOUND of it (last known K + pods inserted since) and its blocks read K on the device;
// the other forms want it known (0 = no one-launch form).
constexpr uint32_t step_k(const StepIn& in) {
  return !in.kinfo_pending ? in.k_host : ((in.step_a_form >= 3u && in.dirs_ready) ? in.k_bound : 0u);
}

// k_fast_step_a (bs_fast.hpp): the one-launch form of launch A + the scan / Filter roles — the latency regime only (<= 256 class slots,
// <= 64 table chunks, <= 4 scalar lanes), no instrumentation that needs the legacy launches (work counters, per-launch stamps), and a context
// that has not seen an in-launch hand-over time out.  BS_STEP_A=0 switches it off.
constexpr bool step_a_possible(const StepIn& in, uint32_t k, uint32_t nchunks) {
  return in.step_a_on && !in.no_fuse_final && k > 0 && k <= kStepSlotsMax && nchunks <= 64 && in.M > 0 && in.P > 0 && !in.collect_stats &&
         in.enable_timing < 2 && in.S <= 4;
}

struct StepAPlan {
  bool ready;                                  // launch it if `grid` blocks are resident at once (K known, or the whole-step form)
  bool whole, ranges;                          // one launch for the whole step | its pod blocks take the load's gang-aligned ranges
  uint32_t qb, pb, nchunks, nshares, fblocks, grid;
  uint32_t launches;                           // 1 (whole) or 2 (k_fast_final behind it)
  uint32_t tk_pods, tk_tab, tk_p1, tk_done;    // the ticket ADVANCES of this launch
};

// K = step_k(in), with in.dirs_ready as it is AFTER the caller's build_dirs.
constexpr StepAPlan step_a_plan(const StepIn& in, uint32_t K) {
  StepAPlan p{};
  p.nshares = geom_max(1u, geom_min(in.step_shares, cdiv(K, 8u)));
  p.fblocks = in.run_filter ? filter_blocks(in.filter_waves, cdiv(2u * K, 64u), in.W) : 0u;
  // forms 2 and 3: class_slots_block publishes every class's slots from the class directory, the pod blocks gate nobody
  p.pb = (in.step_a_form >= 2u && in.dirs_ready) ? cdiv(K, kTblChunk) : 0u;
  // form 3: the pod blocks go on to the final verdicts inside the same launch; its table rows are the nodes in list order (skipped nodes
  // are rows that add nothing), not the compacted rows
  const uint32_t nch_nodes = geom_max(1u, cdiv(in.N, 256u));
  p.whole = in.step_a_form >= 3u && p.pb && nch_nodes <= 64u && in.whole_bufs;
  p.nchunks = p.whole ? nch_nodes : table_chunks(in.M);
  p.ranges = p.whole && in.ranges_valid && in.nranges;
  p.qb = p.ranges ? in.nranges : cdiv(in.P, kTblChunk);
  p.grid = p.qb + p.pb + p.nchunks * p.nshares + p.fblocks;
  p.ready = !in.kinfo_pending || p.whole;
  p.launches = p.whole ? 1u : 2u;
  p.tk_pods = p.pb ? p.pb : p.qb;
  p.tk_tab = p.whole ? 0u : p.nchunks;
  p.tk_p1 = p.whole ? p.qb : 0u;
  p.tk_done = (p.whole && p.qb > kGatherDirectBlocks) ? p.nchunks * p.nshares + p.fblocks : 0u;
  return p;
}

enum class LaunchB : uint32_t {
  kFused,            // scan, Filter and final blocks in one launch (the latency regime, when its whole grid is resident)
  kTwoStreams,       // scan on the side stream, the transposed Filter item on the main one (BS_TP_FILTER=8)
  kTransposed,       // both roles in one launch, Filter by the transposed item (the default of the throughput regime, S <= 4)
  kScanThenFilter,   // the two roles as launches of their own, one stream, the scan first
  kPlain,            // both roles in one launch (k_fast_scan_filter)
};

struct LaunchBPlan {
  LaunchB form;
  bool throughput;                             // more than 16 tiles of class slots
  bool node_words;                             // launch A's grid carries the node-word blocks behind the table chunks
  uint32_t tiles2_min;
  uint32_t nseg, share_b, scan_nsub, scan_blocks, fblocks;
  uint32_t filter_waves;                       // the EFFECTIVE Filter wave count of launch B (FastLaunch::filter_waves)
  uint32_t fused_grid;                         // blocks the fused form needs resident at once
  uint32_t launches;                           // of the chain: launch A, launch B (1 or 2), k_fast_final unless fused
};

// fused_fits: the caller's answer to "are fused_grid blocks resident at once?" — ask with true, and again with false if a kFused plan's
// fused_grid turns out not to fit.
constexpr LaunchBPlan launch_b_plan(const StepIn& in, bool fused_fits = true) {
  LaunchBPlan p{};
  // the regime is known before launch A: an estimate of the class count is enough (the work loops size themselves on the device)
  const uint32_t k_est = geom_min(in.P, in.kinfo_pending ? geom_max(2u * in.h_K, 1024u) : geom_max(in.h_K, 1u));
  // few tiles (the latency regime): one scan item (tile of 64 class slots x share) per BLOCK, its four waves take a quarter of every group's
  // rows each; many tiles (thousands of distinct requests): one item per wave, 4 per block
  const uint32_t tiles = cdiv(k_est, 64u), ftiles = cdiv(2u * k_est, 64u);
  p.throughput = tiles > 16u;
  p.node_words = in.run_filter && p.throughput && in.tp_filter >= 5u && !in.no_nodew && in.have_nodew;
  p.tiles2_min = in.tp_tmin * geom_max(1u, in.nranks);
  // Cap on the shares (blocks of four waves, a quarter of every group's rows each) that deal the live 64-row groups of one tile among
  // themselves: a share that has no group of its own still pays the launch's first round trip — eight is enough (tools/share_sweep.sh)
  p.nseg = in.scan_share ? in.scan_share : 8u;
  // scan shares per tile when an item is one wave's: thousands of tiles are parallelism enough, and every item pays the table's first fetch
  p.share_b = in.tp_share ? in.tp_share : (p.throughput ? 2u : 64u);
  // the Filter work of the transposed item is cut for twice the waves from 65 536 (tile, two node blocks) units on (half of the slot tiles
  // belong to the carried leader and are usually idle: 8192 items leave half of the wave slots without work there)
  p.filter_waves = in.filter_waves;
  if (p.throughput && in.tp_filter >= 5u && !in.filter_waves_env)
    p.filter_waves = in.tp_fwaves ? in.tp_fwaves
                                  : ((uint64_t)ftiles * geom_max(1u, cdiv(in.W, 2u)) >= 65536u ? geom_max(in.filter_waves, 16384u) : in.filter_waves);
  p.fblocks = in.run_filter ? filter_blocks(p.filter_waves, ftiles, in.W) : 0u;
  const uint32_t items4 = tiles * geom_min(p.nseg, cdiv(in.M, 64u)), items1 = cdiv(tiles * geom_min(p.share_b, cdiv(in.M, 64u)), 4u);
  const uint32_t cap = cdiv(in.target_waves, 4u);
  p.fused_grid = geom_max(1u, geom_min(cap, items4)) + p.fblocks + cdiv(in.P, 256u);
  // the fused form (final blocks wait for the producers INSIDE the launch) only in the latency regime, and only when every block of its
  // grid is resident at once; BS_NO_FUSE_FINAL=1 forces the separate launches
  const bool fused = tiles <= 16u && !in.no_fuse_final && fused_fits;
  p.scan_nsub = fused ? 4u : 1u;
  p.scan_blocks = geom_max(1u, geom_min(cap, fused ? items4 : items1));
  const bool split = p.fblocks && p.throughput;
  p.form = fused                                          ? LaunchB::kFused
           : (in.tp_filter == 8u && split)                ? LaunchB::kTwoStreams
           : (in.tp_filter >= 6u && split && in.S <= 4u)  ? LaunchB::kTransposed
           : (in.tp_filter && split)                      ? LaunchB::kScanThenFilter
                                                          : LaunchB::kPlain;
  p.launches = fused ? 2u : ((p.form == LaunchB::kTwoStreams || p.form == LaunchB::kScanThenFilter) ? 4u : 3u);
  return p;
}

}  // namespace bs
