// bs_seq.hpp — the reference's scheduling cycle POD BY POD, resident on the device (bs_seq_run).
//
// What upstream's scheduleOne does with the plugin, for every pending pod in queue order:
//   PreFilter  core.go:88-167    deny / permitted entries, fillOccupiedObj (:477-512), findMaxPG (:701-739), the node scan
//                                compareClusterResourceAndRequire (:595-632) against the CURRENT node requests
//   [Filter    core.go:170-191, :514-564 on every node, when the stage is on]
//   node choice + assume         first fit in list order (the rule host/bs_drain.cpp states; the CPU replay the tests use
//                                restates it), requested += request
//   Permit     core.go:268-309   matched + 1 (:290), quorum (:303), latch (:305)
//   release    batchscheduler.go:254-344 + PostBind core.go:327: the waiting pods of the gang bind, Status.Scheduled += k
// Every pod's decision depends on what the pods before it did to the nodes and the group counters, so the pass is ONE
// persistent workgroup (512 threads, 8 waves) that walks the queue; the O(nodes) and O(groups) parts of a step are
// data-parallel inside it:
//   * findMaxPG is a block maximum over 64-bit keys (progress + 1) << 32 | (inverted index << 1) | "fully scheduled" kept in
//     LDS; one key changes per Permit / capture / release, and the fold is only repeated after such a change.  The tie rule
//     of :729-731 is walked exactly only when the winner is fully scheduled.
//   * singleNodeResource (:634-670) is kept as two resident arrays left07 / left10 = int64(float32(allocatable) * percent) -
//     requested (allocatable never changes during a pass; an assume step patches one node), so the node scan reads ONE
//     int64 per resource lane and node.  The scan goes over the list in ROUNDS of 16 tiles of 64 nodes (one tile per wave):
//     DPP wave scans give the running sums inside a tile (v_add_co_u32_dpp / v_addc_co_u32_dpp: the shift rides on the add),
//     the 16 tile totals are exchanged through LDS (one barrier per round, LDS-only fences so that the next round's loads
//     stay in flight across it), and the pass stops at the round of the first row that covers the request — the reference's
//     early exit (:623-627).
//   * the first-fit choice looks only at tiles whose per-tile bound (max free cpu / memory over schedulable nodes, kept in
//     LDS, tightened whenever a tile was looked at in vain) can hold the pod; the lane that owns the chosen node performs the
//     assume step from the registers it already holds.
//   * the control flow of a pod (a few dozen scalar decisions) runs redundantly in every wave from wave-uniform loads:
//     no broadcast step, and the block only meets at the barriers the reductions need anyway.
// Mutable state read at wave-uniform addresses (group counters / flags / MinResources / OccupiedBy) is read with vector loads
// only (relaxed atomics at workgroup scope: never through the scalar cache, which this kernel's own stores do not update) and
// written by one thread; all waves of a workgroup share the CU's L1, so a barrier orders them.  READ PHASE / WRITE PHASE
// discipline: between the barrier at the top of a pod and the end of its node scan nothing is written (except inside the
// barrier-bracketed capture step); behind it only thread 0 (and the lane that owns the chosen node) write, and nobody else
// reads mutable global state until the next pod's top barrier.
#pragma once

#include "bs_kernels.hpp"
#include "bs_nom_view.hpp"
#include "bs_seq_score.hpp"
#include "bs_seq_sample.hpp"

namespace bs {

#ifndef BS_SEQ_BLOCK
#define BS_SEQ_BLOCK 512
#endif
// Threads of the one workgroup (a multiple of 64, at most 1024).  Measured (tools/seq_bench.py --probe, profiles/r04_*): the pass is
// instruction-issue bound on ONE CU — every wave repeats the pod's control flow, and rocprofv3 counts ~11 000 wave-instructions per
// pod at 16 waves — so fewer waves win until the parallel parts (tile checks, table builds) run short of them: 16 waves 98 ms,
// 8 waves 48 ms, 4 waves 47 ms for cfg3/tail, 8 ahead of 4 on cfg4.
constexpr int kSeqBlock = BS_SEQ_BLOCK;
constexpr int kSeqWaves = kSeqBlock / 64;
constexpr uint32_t kSeqKeysLds = 8192;     // groups whose findMaxPG keys fit the LDS window (64 KB)
constexpr uint32_t kSeqPruneTiles = 1024;  // 64-node tiles whose first-fit bounds fit the LDS window (65 536 nodes)
constexpr uint32_t kSeqWaitList = 512;     // waiting pods of the current gang kept in LDS
constexpr uint32_t kSeqHasRecord = 0x80000000u;   // in nwait[g]: the gang has been released in this pass (it has a release record)
constexpr uint32_t kSeqCursorBits = 9;     // first-fit cursors in LDS: 512 direct-mapped entries (12 bytes each)
constexpr uint32_t kSeqCursors = 1u << kSeqCursorBits;
#ifndef BS_SEQ_RESULT_WAVE
#define BS_SEQ_RESULT_WAVE 1
#endif
constexpr uint32_t kSeqResultThread = kSeqWaves > BS_SEQ_RESULT_WAVE ? 64u * BS_SEQ_RESULT_WAVE : 0u;   // the thread that writes a pod's PreFilter results
#ifndef BS_SEQ_POD_WIN
#define BS_SEQ_POD_WIN 64
#endif
constexpr uint32_t kSeqPodWin = BS_SEQ_POD_WIN;        // pods whose (immutable) input fields are staged in LDS ahead of their turn
#ifndef BS_SEQ_CACHE_MAX
#define BS_SEQ_CACHE_MAX 4
#endif
constexpr uint32_t kSeqCacheSlots = BS_SEQ_CACHE_MAX;     // table summaries (fit class x percent) kept in LDS at most

struct SeqDev {
  // resident state the pass mutates
  int64_t* nreq;                 // [L][stride] node requests
  uint32_t* rpres;               // [n]
  uint32_t* g_matched; uint32_t* g_sc; uint8_t* g_flags; uint32_t* g_cls; int64_t* g_minres; uint32_t* g_mrpres; uint64_t* g_occ;
  // scratch
  int64_t* left07; int64_t* left10;  // [L][stride] int64(float32(allocatable) * 0.7 | 1.0) - requested (core.go:656-659,667)
  uint32_t* nmeta;               // [n] bit 0: a row of the scan (not skipped, core.go:606-617), bit 1: taint error (:639-641), bits 4..: scalar keys of singleNodeResource (:662-668)
  unsigned long long* keys;      // [G] findMaxPG keys when G > kSeqKeysLds
  unsigned long long* wait_rec;  // [P] waiting pod: (next waiting pod of its gang + 1) << 32 | node it was assumed on
  uint32_t* head;                // [G] last waiting pod of the gang + 1, 0 = none
  uint32_t* nwait;               // [G]
  uint32_t* slot_of;             // [G] release record of a gang that is through
  unsigned long long* t_first;   // [G] clock when the gang's first pod entered PreFilter, ~0 = not yet
  const uint32_t* pclass;        // [P] request class of the pod (equal request lanes + present bits <=> equal class; derived at the pod load)
  // results
  uint8_t* pf_code; int32_t* pod_node; uint32_t* pf_first_k; int32_t* pf_leader;
  uint8_t* last_permitted;       // [P] prm.filter_deny: 1 = the pass left a lastPermittedPod entry for the pod (core.go:188)
  uint32_t* released_group; uint32_t* released_pods; unsigned long long* first_tick; unsigned long long* ready_tick;
  uint32_t cap;
  unsigned long long* info;      // [0] gangs released [1] clock ticks of the pass [2] first-fit searches [3] node scans [4] sop leader at the end + 1
                                 // [5] scan rounds executed [6] tiles the first-fit searches looked at [7] findMaxPG folds
};

// Probe build only (-DBS_SEQ_PROBE, tools/seq_bench.py --probe; never the shipped library): shader-clock cycles per phase of a
// pod, summed over the pass, in info[8..15]: control (state in registers / group loads), capture, findMaxPG fold, scan,
// first fit + assume, Permit / release, the top barrier.
#ifdef BS_SEQ_PROBE
#define BS_SEQ_T(k) do { const unsigned long long _t = (unsigned long long)__builtin_readcyclecounter(); ph[k] += _t - tl; tl = _t; } while (0)
#else
#define BS_SEQ_T(k) ((void)0)
#endif

// ... and a finer split (thread 0's clock, kept in LDS so that it costs the kernel no registers): info[32 + k]
#ifdef BS_SEQ_PROBE
#define BS_SEQ_P(k) do { if (threadIdx.x == 0) { const unsigned long long _t = (unsigned long long)__builtin_readcyclecounter(); sh_.ph2[k] += _t - sh_.tl2; sh_.tl2 = _t; } } while (0)
#else
#define BS_SEQ_P(k) ((void)0)
#endif

#ifdef BS_SEQ_PROBE
__device__ unsigned long long g_seq_scan_ph[8];
#define BS_SCAN_T(k) do { if (threadIdx.x == 0) { const unsigned long long _t = (unsigned long long)__builtin_readcyclecounter(); g_seq_scan_ph[k] += _t - stl; stl = _t; } } while (0)
#else
#define BS_SCAN_T(k) ((void)0)
#endif

struct SeqParams {
  uint32_t S, eph_gate, run_filter, C;
  int32_t sop_leader0;           // sop.maxFinishedPG carried into the pass (-1 none)
  uint32_t keys_in_lds, prune;
  uint32_t cache_slots;          // table summaries kept in LDS (0: every scan walks the node list in rounds)
  uint32_t cache_off;            // byte offset of the summary area in dynamic LDS (behind the key window)
  uint32_t use_cursor;           // first-fit cursors per request class (SeqShared::cur_kn, see k_seq_pass's node choice)
  uint32_t filter_deny;          // BS_BATCH_FILTER_DENY: Filter's TTL writes (core.go:183-188) happen inside the pass, every node offered
};

// bs_seq_run_nominated (include/bsched.h, rule S): what the NOM instantiations of k_seq_pass get on top.  The node choice of pod i of
// priority P tests node k with its current requests plus every LIVE row of the nominated-pod table on k with priority >= P that is not
// pod i's own; a row stops being live the moment its pod is assumed (consumed[row] = 1: the flag[] k_nm_move reads behind the pass).
// The sums exist in the fit test only: the assume step, the left arrays, the scan and the first-fit bounds work on the raw requests.
struct SeqNom {
  const NomView* view;           // the table (null: no rows)
  uint32_t rows;
  uint8_t* consumed;             // [rows] zeroed before the launch
  uint32_t* c_pod;               // [rows] of a consumed row: the queue index of its pod ...
  uint32_t* c_node;              // [rows] ... and the node it was assumed on
  const int32_t* pprio;          // [P] priority of queue pod i
  const uint32_t* pown;          // [P] row INDEX of the pod's own nomination, kNmNone = none
  uint32_t lds_off;              // byte offset of SeqNomShared in dynamic LDS (behind the key window and the table summaries)
};
// NOM-only LDS state, in the DYNAMIC part (SeqShared keeps its size: the host's LDS budget and the flag-less instantiations depend on it)
struct SeqNomShared {
  int32_t pw_prio[kSeqPodWin];   // staged with the pod window
  uint32_t pw_own[kSeqPodWin];
  int32_t cur_prio[kSeqCursors]; // priority of the pod that left the first-fit cursor (see cur_ok in k_seq_pass)
  uint32_t grow;                 // a row may GROW the room some pod sees (a negative or huge lane, a sum that could wrap): the pass runs without cursors
  uint32_t wild[kSeqPruneTiles / 32];   // tiles whose first-fit bounds are never used: a row sum there may GROW the room (negative or huge lanes)
};
// bs_seq_run_scored (include/bsched.h, rule P): what the scored instantiations k_seq_scored get on top.  The node choice is a FULL search:
// of the nodes bs_seq_run's rule accepts, the one with the largest total (bs_seq_score.hpp), ties to the lowest index.  Nothing else moves.
constexpr int kSeqScoredFullLanes = 4;     // scalar lanes up to which k_seq_scored keeps everything in registers (see seq_pick_scored; = kLanesUnrolled)
struct SeqScore {
  uint32_t w_least, w_most, w_balanced;
  uint32_t* total;               // [P] zeroed before the launch: the chosen node's total
  uint32_t* n_fit;               // [P] zeroed before the launch: nodes the rule accepted
  uint32_t lds_off;              // byte offset of SeqScoreShared in dynamic LDS (behind the key window and the table summaries)
};
// scored-only LDS state, in the DYNAMIC part as SeqNomShared is
struct SeqScoreShared {
  unsigned long long key[kSeqWaves];   // each wave's best candidate: total << 32 | (0xFFFFFFFF - node), 0 = none
  uint32_t nfit[kSeqWaves];            // candidates the wave counted
};
// bs_seq_run_scored_sampled / bs_seq_run_scored_nominated_sampled (include/bsched.h, rule F): what the sampled instantiations k_seq_sampled /
// k_seq_sampled_nom get on top of SeqScore.  The node choice is an ORDERED walk from a cursor that rotates from pod to pod; it stops behind
// the K-th candidate (at the (K+1)-th, which is not kept) and scores the K it kept.  See seq_pick_sampled.
struct SeqSample {
  uint32_t K;                    // nodes to find, normalised (sample_k): 1 .. N, N = every candidate
  uint32_t s0;                   // the cursor of the first pod (sample_start)
  uint32_t* start;               // [P] zeroed before the launch: the cursor the pod's walk began at
  uint32_t* visited;             // [P] zeroed before the launch: V, the nodes the pod's walk visited
  uint32_t* next;                // [1] zeroed before the launch: the cursor behind the last pod
  uint32_t lds_off;              // byte offset of SeqSampleShared in dynamic LDS (behind SeqScoreShared)
};
// sampled-only LDS state, in the DYNAMIC part as SeqScoreShared is.  cnt[b][w]: the members of C wave w found in its tile of a round of parity
// b — written by lane 0 of wave w in front of the round's barrier, read by every wave behind it; the next writer of the same word is wave w two
// rounds later, behind the next round's barrier, which every reader of this round has reached by then.  vstop: the visit position of the
// (K+1)-th member — written by lane 0 of the one wave whose tile holds it, in the round that stops the walk, read by every wave behind the
// barrier of the block reduction that follows the walk.
struct SeqSampleShared {
  uint32_t cnt[2][kSeqWaves];
  uint32_t vstop;
};

// the rows the fit test adds to node k for a pod of priority P (AddPod per row: all L lanes, wrapping)
template <int TS>
__device__ __forceinline__ void seq_nominees(const NomView& nm, const uint8_t* consumed, uint32_t head, int32_t P, uint32_t own, Shape<TS> sh,
                                             int64_t (&add)[BS_MAX_LANES]) {
  for (uint32_t r = head; r != kNmNone; r = nm.nnext[r]) {
    if (nm.nprio[r] < P || r == own || __hip_atomic_load(&consumed[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
      if (j < sh.L()) add[j] = wadd(add[j], nm.nreq[(size_t)j * nm.nstride + r]);
  }
}

// ... and the same sum for ONE lane j (the lean scored search under rule SP: a walk per lane the pod asks for, nothing kept)
__device__ __forceinline__ int64_t seq_nominees_lane(const NomView& nm, const uint8_t* consumed, uint32_t head, int32_t P, uint32_t own, uint32_t j) {
  int64_t add = 0;
  for (uint32_t r = head; r != kNmNone; r = nm.nnext[r]) {
    if (nm.nprio[r] < P || r == own || __hip_atomic_load(&consumed[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) continue;
    add = wadd(add, nm.nreq[(size_t)j * nm.nstride + r]);
  }
  return add;
}

// ---- wave-uniform loads of state this kernel itself writes: vector loads, value moved to SGPRs ---------------------
__device__ __forceinline__ uint32_t seq_raw32(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t seq_raw8(const uint8_t* p) { return (uint32_t)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint64_t seq_raw64(const void* p) { return __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  const uint32_t lo = uni32((uint32_t)v), hi = uni32((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

#ifdef BS_SEQ_UNSAFE_BARRIERS   // timing experiment only: every barrier LDS-only
#define BS_SEQ_FULL_BARRIER() lds_barrier()
#else
#define BS_SEQ_FULL_BARRIER() __syncthreads()
#endif
// a barrier that orders LDS only: the global loads a wave has in flight (the next round's tile) stay in flight across it
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// 64-bit add with the DPP shift riding on the add itself (two instructions per step instead of two moves + two adds).
// Lanes without a source, and rows masked out, are not written.  The leading s_nop covers the "VALU write -> DPP read"
// hazard of whatever produced the operands (the assembler does not see into inline asm).
#define BS_DPP_ADD64(lo, hi, CTRL) \
  asm volatile("s_nop 1\n\tv_add_co_u32_dpp %0, vcc, %0, %0 " CTRL "\n\tv_addc_co_u32_dpp %1, vcc, %1, %1, vcc " CTRL : "+v"(lo), "+v"(hi) : : "vcc")
__device__ __forceinline__ unsigned long long seq_wave_scan64(unsigned long long v) {        // inclusive, all 64 lanes active
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  BS_DPP_ADD64(lo, hi, "row_shr:1 row_mask:0xf bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_shr:2 row_mask:0xf bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_shr:4 row_mask:0xf bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_shr:8 row_mask:0xf bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_bcast:15 row_mask:0xa bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_bcast:31 row_mask:0xc bank_mask:0xf");
  return ((unsigned long long)hi << 32) | lo;
}
// The same scan for the L resource lanes of a tile at once, STEP-major: the six DPP steps of one lane are a dependent chain
// (each ~10 cycles of issue + hazard), the L chains are independent — interleaved, one chain's wait is the others' issue
// time (the hazard "VALU write -> DPP read" is covered by the 2 L - 1 instructions between two steps of one lane).
#define BS_DPP_ADD64_NN(lo, hi, CTRL) \
  asm volatile("v_add_co_u32_dpp %0, vcc, %0, %0 " CTRL "\n\tv_addc_co_u32_dpp %1, vcc, %1, %1, vcc " CTRL : "+v"(lo), "+v"(hi) : : "vcc")
#define BS_DPP_STEP_ALL(CTRL)                                  \
  _Pragma("unroll") for (uint32_t j = 0; j < BS_MAX_LANES; ++j) \
    if (j < L) BS_DPP_ADD64_NN(lo[j], hi[j], CTRL)
__device__ __forceinline__ void seq_wave_scan64_lanes(unsigned long long (&x)[BS_MAX_LANES], uint32_t L) {   // L >= 4
  uint32_t lo[BS_MAX_LANES], hi[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { lo[j] = (uint32_t)x[j]; hi[j] = (uint32_t)(x[j] >> 32); }
  asm volatile("s_nop 1" ::: "memory");
  BS_DPP_STEP_ALL("row_shr:1 row_mask:0xf bank_mask:0xf");
  BS_DPP_STEP_ALL("row_shr:2 row_mask:0xf bank_mask:0xf");
  BS_DPP_STEP_ALL("row_shr:4 row_mask:0xf bank_mask:0xf");
  BS_DPP_STEP_ALL("row_shr:8 row_mask:0xf bank_mask:0xf");
  BS_DPP_STEP_ALL("row_bcast:15 row_mask:0xa bank_mask:0xf");
  BS_DPP_STEP_ALL("row_bcast:31 row_mask:0xc bank_mask:0xf");
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) x[j] = ((unsigned long long)hi[j] << 32) | lo[j];
}
__device__ __forceinline__ unsigned long long seq_row_scan64(unsigned long long v) {         // inclusive inside each row of 16 lanes
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  BS_DPP_ADD64(lo, hi, "row_shr:1 row_mask:0xf bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_shr:2 row_mask:0xf bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_shr:4 row_mask:0xf bank_mask:0xf");
  BS_DPP_ADD64(lo, hi, "row_shr:8 row_mask:0xf bank_mask:0xf");
  return ((unsigned long long)hi << 32) | lo;
}
// minimum over lanes 0..15 (one value per wave of the block), wave-uniform result
__device__ __forceinline__ uint32_t seq_row_min_u32(uint32_t v) {
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)BS_INF, (int)v, 0x111, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)BS_INF, (int)v, 0x112, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)BS_INF, (int)v, 0x114, 0xF, 0xF, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)BS_INF, (int)v, 0x118, 0xF, 0xF, false));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
}

// A node holds a request for cpu AND memory only if min(free cpu << 20, free memory) >= min(cpu << 20, memory): one number per
// node (1000 millicores ~ 1 GiB) whose tile maximum rules out the tiles in which the free cpu and the free memory sit on
// DIFFERENT nodes — the per-lane maxima alone let those through for ever.
__device__ __forceinline__ long long seq_shl20_sat(long long v) {
  return v > (1ll << 42) ? INT64_MAX : (v < -(1ll << 42) ? INT64_MIN : v * (1ll << 20));
}
__device__ __forceinline__ long long seq_joint(long long cpu, long long mem) {
  const long long c = seq_shl20_sat(cpu);
  return c < mem ? c : mem;
}

// findMaxPG key of one group (core.go:705-717): 0 = not a candidate, ~0 = the uint32 division by zero of :716-717
__device__ __forceinline__ unsigned long long seq_key(uint32_t g, uint32_t flags, uint32_t mm, uint32_t sc, uint32_t matched) {
  if ((flags & BS_GROUP_SCHEDULED_LATCH) || !(flags & BS_GROUP_HAS_POD)) return 0ull;                 // :706-711
  uint32_t fin = 0;
  if ((uint32_t)(mm - sc) != 0u) {                                                                    // :712-714
    if (mm == 0u) return ~0ull;
    fin = (uint32_t)((uint32_t)(matched + sc) * 1000u) / mm;                                          // :716-717
  }
  return (((unsigned long long)fin + 1ull) << 32) | ((unsigned long long)(0x7FFFFFFFu - g) << 1) | (sc >= mm ? 1ull : 0ull);
}

__device__ __forceinline__ unsigned long long wave_max_u64_all(unsigned long long v) {
  // signed DPP maximum on the sign-flipped value; result in every lane
  const long long s = (long long)(v ^ 0x8000000000000000ull);
  const long long m = readlane63_i64(wave_max_i64_lane63(s));
  return (unsigned long long)m ^ 0x8000000000000000ull;
}

struct SeqShared {
  unsigned long long kmax[kSeqWaves];
  uint32_t red[kSeqWaves];
  uint32_t fdw[2][kSeqWaves];                            // Filter's TTL writes: per wave, bit 0 = a node's Filter failed, bit 1 = a node's Filter passed (parity per use)
  unsigned long long tot[2][BS_MAX_LANES][kSeqWaves];   // per round parity: tile totals, lane-major so that lanes 0..15 read one row
  uint32_t wpres[2][kSeqWaves];
  uint32_t fk[2][kSeqWaves];
  unsigned long long cmask[kSeqWaves];                   // first fit: candidate tiles of a chunk of 1024
  uint32_t pick[2][kSeqWaves];
  long long pmax[3][kSeqPruneTiles];                     // per tile, over schedulable nodes: max free cpu, max free memory, max of min(free cpu << 20, free memory)
  uint32_t tight[kSeqPruneTiles / 32];                   // first fit: the tile's bounds are exact (set by the wave that tightened them, cleared by an assume step in the tile)
  uint32_t hit_w[2];                                     // first fit / scan: lowest TILE with a hit so far (nobody looks behind it); searches alternate
                                                         // between the two words, so that a word is re-armed a whole search (a barrier) before its next use
  uint32_t wl_pod[kSeqWaitList], wl_node[kSeqWaitList];  // waiting pods of the CURRENT gang (released in parallel; the chain in global memory is the fallback)
  uint32_t asm_ap[2][kSeqWaves], asm_rp[2][kSeqWaves], asm_fit[2][kSeqWaves];   // first fit: keys / fit bits of each wave's node (see SeqAssumed)
  // first-fit cursors, direct-mapped by (request class, fit class): (request class + 1) << 32 | node the class's last search ended at
  // (nodes: nothing fits any more), and the fit class that search ran under.  In LDS, not in global memory: thread 0 writes a cursor
  // behind the search, the next pod's top barrier (LDS-only) orders it for every wave — all waves read the SAME cursor, which the
  // barriers inside the search rely on.  An entry that was evicted only costs the next search of that class its head start.
  unsigned long long cur_kn[kSeqCursors];
  uint32_t cur_fc[kSeqCursors];
  // the next kSeqPodWin pods' input fields (nothing the pass writes): one bulk fetch per window instead of half a dozen dependent
  // trips to memory per pod — group, flags, fit class, present bits, request class, owner hash, the group's MinMember, request lanes
  int64_t pw_req[BS_MAX_LANES][kSeqPodWin];
  uint64_t pw_owner[kSeqPodWin];
  int32_t pw_group[kSeqPodWin];
  uint32_t pw_flags[kSeqPodWin], pw_cls[kSeqPodWin], pw_pres[kSeqPodWin], pw_pclass[kSeqPodWin], pw_mm[kSeqPodWin];
#ifdef BS_SEQ_PROBE
  unsigned long long ph2[32], tl2;
#endif
};

// ---------------------------------------------------------------------------------------------------------------------
// compareClusterResourceAndRequire (core.go:595-632) against the resident left arrays.  Returns the node index of the
// first row whose running sum covers R (first_k), BS_INF if none; wave-uniform, identical in every wave.
// ---------------------------------------------------------------------------------------------------------------------
template <int TS>
__device__ __forceinline__ uint32_t seq_scan(const NodesDev& nd, const SeqDev& sq, const SeqParams& prm, SeqShared& sh_, uint32_t tcls, bool pct07,
                                             const Res& R, unsigned long long& rounds_done) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), S = sh.S();
  const int lane = lane_id(), w = (int)uni32((uint32_t)wave_id());
  const uint32_t N = nd.n;
  if (!N) return BS_INF;
  const uint32_t ntiles = (N + 63u) >> 6, rounds = (ntiles + kSeqWaves - 1u) / kSeqWaves;
  const int64_t* lf = pct07 ? sq.left07 : sq.left10;
  const uint32_t* fitrow = nd.fit + (size_t)tcls * nd.fit_words;
  BS_SEQ_FULL_BARRIER();                                            // the assume steps of earlier pods (left arrays, meta words) have landed
  struct Tile { int64_t v[BS_MAX_LANES]; uint32_t meta, fitw; };
  auto load_tile = [&](uint32_t r, Tile& t) {
    const uint32_t n = ((r * kSeqWaves + (uint32_t)w) << 6) + (uint32_t)lane;
    const uint32_t nn = n < N ? n : N - 1u;
    t.meta = n < N ? sq.nmeta[nn] : 0u;
    t.fitw = fitrow[nn >> 5];
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
      if (j < L) t.v[j] = lf[(size_t)j * nd.stride + nn];
  };
  Tile cur, nxt;
  load_tile(0, cur);
  nxt = cur;
  unsigned long long carry[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) carry[j] = 0;
  uint32_t pcarry = 0, found = BS_INF;
  uint32_t r = 0;
#ifdef BS_SEQ_PROBE
  unsigned long long stl = (unsigned long long)__builtin_readcyclecounter();
#endif
  for (; r < rounds; ++r) {
    if (r + 1 < rounds) load_tile(r + 1, nxt);
    BS_SCAN_T(0);
    const uint32_t b = r & 1u;
    const uint32_t n = ((r * kSeqWaves + (uint32_t)w) << 6) + (uint32_t)lane;
    const bool row = n < N && (cur.meta & 1u);                                                        // core.go:606-617
    const bool fit = row && !(cur.meta & 2u) && ((cur.fitw >> (n & 31u)) & 1u);                        // :639-645
    const uint32_t pres = fit ? (cur.meta >> 4) : 0u;                                                 // :662-668
    unsigned long long x[BS_MAX_LANES];
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
      const bool live = j < L && fit && (j < 4 || (pres & (1u << (j - 4)))) && !(j == BS_LANE_EPH && !prm.eph_gate);
      x[j] = live ? (unsigned long long)cur.v[j] : 0ull;
    }
    BS_SCAN_T(1);
    seq_wave_scan64_lanes(x, L);                                                                      // running sums inside the tile (:621)
    BS_SCAN_T(2);
    if (lane == 63) {
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
        if (j < L) sh_.tot[b][j][w] = x[j];
    }
    unsigned long long km[BS_MAX_SCALARS];
    uint32_t wp = 0;
#pragma unroll
    for (uint32_t s = 0; s < BS_MAX_SCALARS; ++s) {
      km[s] = 0;
      if (s < S) {
        km[s] = __ballot((pres >> s) & 1u);
        if (km[s]) wp |= 1u << s;
      }
    }
    if (lane == 0) sh_.wpres[b][w] = wp;
    BS_SCAN_T(3);
    lds_barrier();
    BS_SCAN_T(4);
    // a hit of the PREVIOUS round is visible now: the reference's loop ended there (early exit, :623-627)
    if (r > 0) {
      const uint32_t prev = seq_row_min_u32(lane < kSeqWaves ? sh_.fk[b ^ 1u][lane] : BS_INF);
      if (prev != BS_INF) { found = prev; break; }
    }
    BS_SCAN_T(5);
    // offsets: row r of the wave (16 lanes) holds the tile totals of resource lane 4 q + r — ONE row scan serves four lanes
    bool ok = row;
    const uint32_t pw = lane < kSeqWaves ? sh_.wpres[b][lane] : 0u;
    uint32_t pbefore = pcarry, pround = 0;
    unsigned long long inc4[BS_MAX_LANES / 4];
#pragma unroll
    for (uint32_t qd = 0; qd < BS_MAX_LANES / 4; ++qd) {
      inc4[qd] = 0;
      if (qd * 4u < L) {
        const uint32_t jr = qd * 4u + ((uint32_t)lane >> 4), wi = (uint32_t)lane & 15u;
        inc4[qd] = seq_row_scan64((jr < L && wi < (uint32_t)kSeqWaves) ? sh_.tot[b][jr][wi] : 0ull);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
      if (j < L) {
        const unsigned long long inc = inc4[j >> 2];
        const int rl = (int)((j & 3u) << 4);
        const unsigned long long off = carry[j] + (w ? readlane_u64(inc, rl + w - 1) : 0ull);
        carry[j] += readlane_u64(inc, rl + kSeqWaves - 1);
        const int64_t sum = (int64_t)(x[j] + off);
        if (j < 4) {
          ok = ok && sum >= R.v[j];                                                                    // :673-685
        } else {
          const uint32_t s = j - 4;
          const unsigned long long bal = __ballot(lane < kSeqWaves && ((pw >> s) & 1u));
          if (bal & ((1ull << w) - 1ull)) pbefore |= 1u << s;
          if (bal) pround |= 1u << s;
          const bool have = ((pbefore >> s) & 1u) || (km[s] & ((2ull << lane) - 1ull));              // the key exists in the running sum
          if ((R.present >> s) & 1u) ok = ok && (have ? !(R.v[j] > sum) : R.v[j] == 0);              // :686-697
        }
      }
    }
    pcarry |= pround;
    BS_SCAN_T(6);
    const unsigned long long m = __ballot(ok);
    if (lane == 0) sh_.fk[b][w] = m ? ((r * kSeqWaves + (uint32_t)w) << 6) + (uint32_t)(__ffsll((long long)m) - 1) : BS_INF;
    cur = nxt;
    BS_SCAN_T(7);
  }
  rounds_done += r < rounds ? r + 1 : rounds;
  if (found == BS_INF) {                                      // the last round's hits
    lds_barrier();
    found = seq_row_min_u32(lane < kSeqWaves ? sh_.fk[(rounds - 1u) & 1u][lane] : BS_INF);
  }
  // (the next writer of tot / wpres / fk is the next scan: the first-fit search's barriers or the next pod's top barrier lie between)
  return found;
}

// ---------------------------------------------------------------------------------------------------------------------
// Table summaries.  For a (fit class, percent) table the scan only has to look INSIDE a tile of 64 nodes when the tile can
// hold the first covering row: with the running sum in front of the tile (OFFSET: the exclusive prefix of the tile totals)
// and the largest running sum inside it per resource lane (MAX LOCAL PREFIX over the rows the reference compares at), a tile
// is a candidate iff offset + max >= request on every lane.  Offsets, totals, maxima and the scalar keys in front of / inside
// a tile are kept in LDS for up to four tables, one thread per tile.  They are MAINTAINED, not recomputed:
//   * an assume step moves the chosen node's left values by the pod's request (the same delta in every table the node
//     counts in): every thread subtracts it from the offsets of the tiles behind the node's — one LDS subtract per lane;
//   * maxima are left alone (requests only grow in a pass, so an old maximum is still an upper bound: more candidates, never
//     fewer) and are TIGHTENED to the exact value by the wave that looked into a candidate tile in vain;
//   * the rare events that would break a bound (a negative request, a scalar key the node's requests did not have) drop the
//     table; it is summarised afresh at its next use.
// A scan is then: candidate test (one thread per tile, LDS only) -> every wave looks into ITS OWN candidate tiles in list order
// until it has a hit (DPP scan of the tile's 64 rows on top of the tile's offset) -> one barrier -> the smallest hit wins.
// A rejected request (no candidate) never touches the node list.  Sums wrap (Go semantics): a tile whose local sums leave
// (-2^62, 2^62), or an offset outside it, is never pruned.
// ---------------------------------------------------------------------------------------------------------------------
struct SeqCache {
  uint32_t T, K;                 // tiles (<= kSeqBlock: one thread per tile), slots
  unsigned long long* tt;        // [K][L][T] tile totals
  unsigned long long* off;       // [K][L][T] running sum in front of the tile
  long long* mp;                 // [K][L][T] max local prefix per lane (INT64_MIN: no row in the tile, INT64_MAX: not prunable)
  uint32_t* pr;                  // [K][T] scalar keys the tile's nodes bring into the running sum
  uint32_t* pb;                  // [K][T] scalar keys present in front of the tile
};
template <int TS>
__device__ __forceinline__ SeqCache seq_cache_view(unsigned char* base, uint32_t T, uint32_t K, Shape<TS> sh) {
  SeqCache c;
  const size_t L = sh.L();
  c.T = T; c.K = K;
  c.tt = reinterpret_cast<unsigned long long*>(base);
  c.off = c.tt + (size_t)K * L * T;
  c.mp = reinterpret_cast<long long*>(c.off + (size_t)K * L * T);
  c.pr = reinterpret_cast<uint32_t*>(c.mp + (size_t)K * L * T);
  c.pb = c.pr + (size_t)K * T;
  return c;
}

// One tile (64 nodes, one wave): live values -> running sums inside the tile.  x[j] = inclusive local sums, row / pres per lane.
template <int TS>
__device__ __forceinline__ void seq_tile_local(const NodesDev& nd, const SeqDev& sq, const SeqParams& prm, const int64_t* lf, const uint32_t* fitrow,
                                               uint32_t tile, unsigned long long (&x)[BS_MAX_LANES], bool& row, uint32_t& pres) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), N = nd.n;
  const uint32_t n = (tile << 6) + (uint32_t)lane_id();
  const uint32_t nn = n < N ? n : N - 1u;
  const uint32_t meta = n < N ? sq.nmeta[nn] : 0u, fitw = fitrow[nn >> 5];
  int64_t v[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
    if (j < L) v[j] = lf[(size_t)j * nd.stride + nn];
  row = n < N && (meta & 1u);                                                                        // core.go:606-617
  const bool fit = row && !(meta & 2u) && ((fitw >> (n & 31u)) & 1u);                                 // :639-645
  pres = fit ? (meta >> 4) : 0u;                                                                     // :662-668
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
    const bool live = j < L && fit && (j < 4 || (pres & (1u << (j - 4)))) && !(j == BS_LANE_EPH && !prm.eph_gate);
    x[j] = live ? (unsigned long long)v[j] : 0ull;
  }
  seq_wave_scan64_lanes(x, L);
}

// exact maxima of a tile's local sums -> the slot's mp (and, when `totals`, its totals and keys): the calling wave holds x / row / pres
template <int TS>
__device__ __forceinline__ void seq_cache_put(const SeqParams& prm, const SeqCache& ch, uint32_t slot, uint32_t tile, const unsigned long long (&x)[BS_MAX_LANES],
                                              bool row, uint32_t pres, bool totals) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), S = sh.S();
  constexpr long long kSafe = 1ll << 62;
  const bool anyrow = __ballot(row) != 0ull;
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
    if (j < L) {
      const long long xi = (long long)x[j];
      const bool risky = __ballot(xi >= kSafe || xi <= -kSafe) != 0ull;
      const long long mx = readlane63_i64(wave_max_i64_lane63(row ? xi : INT64_MIN));
      if (lane_id() == 63) {
        if (totals) ch.tt[((size_t)slot * L + j) * ch.T + tile] = x[j];
        ch.mp[((size_t)slot * L + j) * ch.T + tile] = !anyrow ? INT64_MIN : (risky ? INT64_MAX : mx);
      }
    }
  }
  if (totals) {
    uint32_t wp = 0;
#pragma unroll
    for (uint32_t s2 = 0; s2 < BS_MAX_SCALARS; ++s2)
      if (s2 < S && __ballot((pres >> s2) & 1u)) wp |= 1u << s2;
    if (lane_id() == 0) ch.pr[(size_t)slot * ch.T + tile] = wp;
  }
}

// Summarise a table from scratch into slot `slot`: every tile's totals / maxima / keys, then the offsets and the keys in
// front of every tile (a two-level prefix over the tile totals: one thread per tile).
template <int TS>
__device__ __forceinline__ void seq_cache_build(const NodesDev& nd, const SeqDev& sq, const SeqParams& prm, SeqShared& sh_, const SeqCache& ch, uint32_t slot,
                                                uint32_t tcls, bool pct07) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), S = sh.S();
  const int lane = lane_id(), w = (int)uni32((uint32_t)wave_id());
  const uint32_t T = ch.T;
  const int64_t* lf = pct07 ? sq.left07 : sq.left10;
  const uint32_t* fitrow = nd.fit + (size_t)tcls * nd.fit_words;
  for (uint32_t tile = (uint32_t)w; tile < T; tile += kSeqWaves) {
    unsigned long long x[BS_MAX_LANES];
    bool row;
    uint32_t pres;
    seq_tile_local<TS>(nd, sq, prm, lf, fitrow, tile, x, row, pres);
    seq_cache_put<TS>(prm, ch, slot, tile, x, row, pres, true);
  }
  lds_barrier();
  // offsets and keys in front of every tile: chunks of one tile per thread, the running sums carried from chunk to chunk
  unsigned long long carry[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) carry[j] = 0;
  uint32_t pcarry = 0;
  for (uint32_t chunk = 0; chunk < T; chunk += kSeqBlock) {
    const uint32_t t = chunk + threadIdx.x;
    unsigned long long v[BS_MAX_LANES], inc[BS_MAX_LANES];
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { v[j] = (j < L && t < T) ? ch.tt[((size_t)slot * L + j) * T + t] : 0ull; inc[j] = v[j]; }
    const uint32_t mypr = t < T ? ch.pr[(size_t)slot * T + t] : 0u;
    seq_wave_scan64_lanes(inc, L);
    if (lane == 63) {
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
        if (j < L) sh_.tot[0][j][w] = inc[j];
    }
    uint32_t wp = 0;
#pragma unroll
    for (uint32_t s2 = 0; s2 < BS_MAX_SCALARS; ++s2)
      if (s2 < S && __ballot((mypr >> s2) & 1u)) wp |= 1u << s2;
    if (lane == 0) sh_.wpres[0][w] = wp;
    lds_barrier();
    unsigned long long inc4[BS_MAX_LANES / 4];
#pragma unroll
    for (uint32_t qd = 0; qd < BS_MAX_LANES / 4; ++qd) {
      inc4[qd] = 0;
      if (qd * 4u < L) {
        const uint32_t jr = qd * 4u + ((uint32_t)lane >> 4), wi = (uint32_t)lane & 15u;
        inc4[qd] = seq_row_scan64((jr < L && wi < (uint32_t)kSeqWaves) ? sh_.tot[0][jr][wi] : 0ull);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
      if (j < L) {
        const int rl = (int)((j & 3u) << 4);
        const unsigned long long woff = w ? readlane_u64(inc4[j >> 2], rl + w - 1) : 0ull;
        if (t < T) ch.off[((size_t)slot * L + j) * T + t] = carry[j] + inc[j] - v[j] + woff;
        carry[j] += readlane_u64(inc4[j >> 2], rl + kSeqWaves - 1);
      }
    }
    const uint32_t pw = (uint32_t)lane < (uint32_t)kSeqWaves ? sh_.wpres[0][lane] : 0u;
    uint32_t pbt = pcarry, pround = 0;
#pragma unroll
    for (uint32_t s2 = 0; s2 < BS_MAX_SCALARS; ++s2) {
      if (s2 < S) {
        const unsigned long long bal = __ballot((uint32_t)lane < (uint32_t)kSeqWaves && ((pw >> s2) & 1u));
        const unsigned long long km = __ballot((mypr >> s2) & 1u);
        if ((bal & ((1ull << w) - 1ull)) || (km & ((1ull << lane) - 1ull))) pbt |= 1u << s2;
        if (bal) pround |= 1u << s2;
      }
    }
    if (t < T) ch.pb[(size_t)slot * T + t] = pbt;
    pcarry |= pround;
    lds_barrier();
  }
}

// compareClusterResourceAndRequire through the summaries of slot `slot`.  first_k or BS_INF; wave-uniform, same in every wave.
template <int TS>
__device__ __forceinline__ uint32_t seq_scan_cached(const NodesDev& nd, const SeqDev& sq, const SeqParams& prm, SeqShared& sh_, const SeqCache& ch, uint32_t slot,
                                                    uint32_t tcls, bool pct07, const Res& R, uint32_t& hit_par, unsigned long long& rounds_done) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L();
  const int lane = lane_id(), w = (int)uni32((uint32_t)wave_id());
  const uint32_t T = ch.T;                                       // tiles; thread tid tests tiles tid, tid + block, ...
  const uint32_t hp = hit_par;
  hit_par ^= 1u;
  constexpr long long kSafe = 1ll << 62;
  const int64_t* lf = pct07 ? sq.left07 : sq.left10;
  const uint32_t* fitrow = nd.fit + (size_t)tcls * nd.fit_words;
  uint32_t mine = BS_INF;
  for (uint32_t chunk = 0; chunk < T && mine == BS_INF; chunk += kSeqBlock) {
    // ---- candidate test, LDS only
    const uint32_t t = chunk + threadIdx.x;
    bool cand = t < T;
    if (t < T) {
      const uint32_t mypr = ch.pr[(size_t)slot * T + t], mypb = ch.pb[(size_t)slot * T + t];
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        if (j < L) {
          const long long off = (long long)ch.off[((size_t)slot * L + j) * T + t];
          const long long m = ch.mp[((size_t)slot * L + j) * T + t];
          const bool open = m == INT64_MAX || off >= kSafe || off <= -kSafe;         // not prunable on this lane
          const bool reach = m != INT64_MIN && (open || off + m >= R.v[j]);
          if (j < 4) cand = cand && reach;
          else if ((R.present >> (j - 4)) & 1u) {
            if ((mypb >> (j - 4)) & 1u) cand = cand && reach;                         // the key is in the running sum in front of the tile
            else if (!((mypr >> (j - 4)) & 1u)) cand = cand && R.v[j] == 0 && m != INT64_MIN;   // ... at no row of the tile
            else cand = cand && m != INT64_MIN;                                       // ... appears inside the tile: look
          } else cand = cand && m != INT64_MIN;
        }
      }
    }
    unsigned long long cm = __ballot(cand);
    BS_SEQ_P(5);
    // ---- this wave's candidate tiles of the chunk, in list order, until one holds a covering row
    while (cm && mine == BS_INF) {
      const uint32_t tile = chunk + ((uint32_t)w << 6) + (uint32_t)(__ffsll((long long)cm) - 1);
      cm &= cm - 1ull;
      if (uni32(__hip_atomic_load(&sh_.hit_w[hp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < tile) { cm = 0; chunk = T; break; }   // a covering row in front of this tile exists
      rounds_done++;
      unsigned long long x[BS_MAX_LANES];
      bool row;
      uint32_t pres;
      seq_tile_local<TS>(nd, sq, prm, lf, fitrow, tile, x, row, pres);
      const uint32_t pbt = ch.pb[(size_t)slot * T + tile];
      bool ok = row;
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        if (j < L) {
          const int64_t sum = (int64_t)(x[j] + ch.off[((size_t)slot * L + j) * T + tile]);
          if (j < 4) ok = ok && sum >= R.v[j];                                                         // core.go:673-685
          else {
            const uint32_t s2 = j - 4;
            const unsigned long long km = __ballot((pres >> s2) & 1u);
            const bool have = ((pbt >> s2) & 1u) || (km & ((2ull << lane) - 1ull));
            if ((R.present >> s2) & 1u) ok = ok && (have ? !(R.v[j] > sum) : R.v[j] == 0);            // :686-697
          }
        }
      }
      const unsigned long long m = __ballot(ok);
      if (m) {
        mine = (tile << 6) + (uint32_t)(__ffsll((long long)m) - 1);
        if (lane == 0) __hip_atomic_fetch_min(&sh_.hit_w[hp], tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else seq_cache_put<TS>(prm, ch, slot, tile, x, row, pres, false);      // looked at in vain: the tile's maxima become exact
    }
  }
  BS_SEQ_P(6);
  if (lane == 0) sh_.fk[0][w] = mine;
  lds_barrier();
  if (threadIdx.x == 0) sh_.hit_w[hp] = BS_INF;               // (re-armed behind the barrier; the NEXT search uses the other word)
  const uint32_t fk_all = seq_row_min_u32(lane < kSeqWaves ? sh_.fk[0][lane] : BS_INF);
  BS_SEQ_P(7);
  return fk_all;
}

// ---------------------------------------------------------------------------------------------------------------------
// first fit in list order + the assume step (upstream's node choice / cache.AssumePod, restated; see bs_drain.cpp).
// Returns the node (BS_INF none), wave-uniform, identical in every wave.  Every wave looks into ITS OWN candidate tiles
// (per-tile bound on free cpu / memory, LDS) in list order until it has a node; the smallest one wins; the lane that owns
// it rewrites the node's request lanes, left values and meta word, and what the other waves need to follow the change in the
// table summaries (the node's keys and fit bits) has been published before the barrier that decides.
// ---------------------------------------------------------------------------------------------------------------------
struct SeqPick {
  uint32_t pcls;                 // the pod's own fit class
  int64_t preq[BS_MAX_LANES];    // raw request lanes of the pod
  uint32_t ppres;
  uint32_t fl;                   // Filter (computeResourceSatisfied) of the pod, BS_FL_* (PASS_NOT_GROUPED when the stage is off)
  uint32_t ff;                   // bit0: case 2 impossible, bit1: the leader's member cannot be "held" (scalar key)
  int64_t FR[4], FM[4];
};
struct SeqAssumed { uint32_t ap, rp, fitbits; };     // of the chosen node: allocatable keys, request keys BEFORE the step, bit c = fits the class of slot c

struct SeqPickNom { const SeqNom* nom; const SeqNomShared* ns; int32_t prio; uint32_t own; };   // NOM only: the pod's priority and own row
template <int TS, bool NOM>
__device__ __forceinline__ uint32_t seq_pick(const NodesDev& nd, const SeqDev& sq, const SeqParams& prm, SeqShared& sh_, const SeqPick& q,
                                             const uint32_t (&slot_key)[kSeqCacheSlots], bool drained, uint32_t& hit_par, SeqAssumed& out,
                                             unsigned long long& tiles_looked, uint32_t start_tile, const SeqPickNom& pn) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), S = sh.S();
  const int lane = lane_id(), w = (int)uni32((uint32_t)wave_id());
  const uint32_t N = nd.n;
  out.ap = out.rp = out.fitbits = 0;
  if (!N || q.pcls >= nd.n_classes || q.fl >= 16u) return BS_INF;          // (ERR_PG_NOT_FOUND / the nil-leader panic: Filter fails everywhere)
  const bool fl_all = q.fl != BS_FL_EVALUATED;                              // Filter passes on every node
  const uint32_t ntiles = (N + 63u) >> 6;
  const uint32_t* fitrow = nd.fit + (size_t)q.pcls * nd.fit_words;
  uint32_t found = BS_INF;
  const uint32_t pb = 0, hp = hit_par;
  hit_par ^= 1u;
  if (!drained) __syncthreads();                                            // the assume steps of earlier pods have landed before a tile is read
  BS_SEQ_P(10);
  uint32_t mine = BS_INF;
  int64_t al[BS_MAX_LANES], rq[BS_MAX_LANES], l07[BS_MAX_LANES], l10[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { al[j] = 0; rq[j] = 0; l07[j] = 0; l10[j] = 0; }
  uint32_t ap = 0, rp = 0, fbits = 0, meta = 0;
  // start_tile: the first-fit cursor of the pod's request class — an identical request, with the same fit class, last ended its search
  // there; while requests only ADD to the nodes nothing in front of it can have started to fit (k_seq_pass keeps that invariant)
  for (uint32_t chunk = (start_tile / kSeqBlock) * kSeqBlock; chunk < ntiles && mine == BS_INF; chunk += kSeqBlock) {
    const uint32_t t = chunk + threadIdx.x;
    bool cand = t < ntiles && t >= start_tile;
    if (cand && prm.prune) {
      cand = !(q.preq[0] > 0 && sh_.pmax[0][t] < q.preq[0]) && !(q.preq[1] > 0 && sh_.pmax[1][t] < q.preq[1]);
      if (q.preq[0] > 0 && q.preq[1] > 0) cand = cand && !(sh_.pmax[2][t] < seq_joint(q.preq[0], q.preq[1]));
    }
    unsigned long long cm = __ballot(cand);
    while (cm && mine == BS_INF) {
      const uint32_t tile = chunk + ((uint32_t)w << 6) + (uint32_t)(__ffsll((long long)cm) - 1);
      cm &= cm - 1ull;
      if (uni32(__hip_atomic_load(&sh_.hit_w[hp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) < tile) { cm = 0; chunk = ntiles; break; }   // a node in front of this tile takes the pod
      tiles_looked++;
      const uint32_t n = (tile << 6) + (uint32_t)lane;
      const bool valid = n < N;
      const uint32_t nn = valid ? n : N - 1u;
      const uint32_t fl = nd.flags[nn];
      ap = nd.apres[nn];
      rp = sq.rpres[nn];
      const uint32_t fw = fitrow[nn >> 5];
      uint32_t fws[kSeqCacheSlots];
#pragma unroll
      for (uint32_t c = 0; c < kSeqCacheSlots; ++c)
        fws[c] = (c < prm.cache_slots && slot_key[c] != BS_INF) ? nd.fit[(size_t)(slot_key[c] >> 1) * nd.fit_words + (nn >> 5)] : 0u;
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        if (j < L) {
          al[j] = nd.alloc[(size_t)j * nd.stride + nn];
          rq[j] = sq.nreq[(size_t)j * nd.stride + nn];
          l07[j] = sq.left07[(size_t)j * nd.stride + nn];       // (for the assume step: no second round trip behind the decision)
          l10[j] = sq.left10[(size_t)j * nd.stride + nn];
        }
      }
      meta = sq.nmeta[nn];
      fbits = 0;
#pragma unroll
      for (uint32_t c = 0; c < kSeqCacheSlots; ++c) fbits |= ((fws[c] >> (nn & 31u)) & 1u) << c;
      const bool sched = valid && fl == 0u;
      bool ok = sched && ((fw >> (nn & 31u)) & 1u);
      const int64_t f0 = wsub(al[0], rq[0]), f1 = wsub(al[1], rq[1]);
      if constexpr (NOM) {
        // rule S: the fit test sees the node's requests plus the live rows on it (a LOCAL sum: the assume step and the bounds below keep
        // reading the raw rq / l07 / l10).  Lanes without rows take one branch.
        int64_t add[BS_MAX_LANES];
#pragma unroll
        for (uint32_t j = 0; j < BS_MAX_LANES; ++j) add[j] = 0;
        if (pn.nom->view) {
          const NomView nm = *pn.nom->view;
          const uint32_t head = valid ? nm.nhead[nn] : kNmNone;
          if (head != kNmNone) seq_nominees<TS>(nm, pn.nom->consumed, head, pn.prio, pn.own, sh, add);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) ok = ok && !(q.preq[j] > 0 && q.preq[j] > wsub(al[j], wadd(rq[j], add[j])));
        ok = ok && !(wadd(wadd(rq[3], add[3]), 1) > al[3]);
#pragma unroll
        for (uint32_t s = 0; s < BS_MAX_SCALARS; ++s) {
          if (s < S && ((q.ppres >> s) & 1u) && q.preq[4 + s] > 0) {
            const int64_t r0 = wadd(((rp >> s) & 1u) ? rq[4 + s] : 0, add[4 + s]);
            ok = ok && ((ap >> s) & 1u) && !(q.preq[4 + s] > wsub(al[4 + s], r0));
          }
        }
      }
      if (!fl_all) {                                         // computeResourceSatisfied on this node (core.go:545-563)
        bool c2 = !(q.ff & 1u), c3h = !(q.ff & 2u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t left = wsub(al[j], rq[j]);                                                   // getLeftResource :460-463
          c2 = c2 && left >= q.FR[j];
          c3h = c3h && left >= q.FM[j];
        }
        ok = ok && (c2 || !c3h);                                                                     // case 2 | case 3
      }
      if constexpr (!NOM) {
#pragma unroll
      for (int j = 0; j < 3; ++j) ok = ok && !(q.preq[j] > 0 && q.preq[j] > wsub(al[j], rq[j]));
      ok = ok && !(wadd(rq[3], 1) > al[3]);
#pragma unroll
      for (uint32_t s = 0; s < BS_MAX_SCALARS; ++s) {
        if (s < S && ((q.ppres >> s) & 1u) && q.preq[4 + s] > 0) {
          const int64_t r0 = ((rp >> s) & 1u) ? rq[4 + s] : 0;
          ok = ok && ((ap >> s) & 1u) && !(q.preq[4 + s] > wsub(al[4 + s], r0));
        }
      }
      }
      const unsigned long long m = __ballot(ok);
      if (m) {
        mine = (tile << 6) + (uint32_t)(__ffsll((long long)m) - 1);
        if (lane == 0) __hip_atomic_fetch_min(&sh_.hit_w[hp], tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else if (prm.prune && !((sh_.tight[tile >> 5] >> (tile & 31u)) & 1u)) {   // looked at in vain: tighten the tile's bounds to what is really there
        const long long m0 = readlane63_i64(wave_max_i64_lane63(sched ? (long long)f0 : INT64_MIN));
        const long long m1 = readlane63_i64(wave_max_i64_lane63(sched ? (long long)f1 : INT64_MIN));
        const long long m2 = readlane63_i64(wave_max_i64_lane63(sched ? seq_joint(f0, f1) : INT64_MIN));
        if constexpr (NOM) {                                 // (not a wild tile's: its bounds stay open, see the prologue of the pass)
          if (lane == 0 && !((pn.ns->wild[tile >> 5] >> (tile & 31u)) & 1u)) { sh_.pmax[0][tile] = m0; sh_.pmax[1][tile] = m1; sh_.pmax[2][tile] = m2; atomicOr(&sh_.tight[tile >> 5], 1u << (tile & 31u)); }
        } else {
          if (lane == 0) { sh_.pmax[0][tile] = m0; sh_.pmax[1][tile] = m1; sh_.pmax[2][tile] = m2; atomicOr(&sh_.tight[tile >> 5], 1u << (tile & 31u)); }
        }
      }
    }
  }
  BS_SEQ_P(11);
  {
    const bool owner = mine != BS_INF && (uint32_t)lane == (mine & 63u);
    if (owner) { sh_.pick[pb][w] = mine; sh_.asm_ap[pb][w] = ap; sh_.asm_rp[pb][w] = rp; sh_.asm_fit[pb][w] = fbits; }
    if (mine == BS_INF && lane == 0) sh_.pick[pb][w] = BS_INF;
    lds_barrier();
    const uint32_t mypick = lane < kSeqWaves ? sh_.pick[pb][lane] : BS_INF;
    found = seq_row_min_u32(mypick);
    if (found != BS_INF) {
      const unsigned long long wm = __ballot(mypick == found);               // the wave that holds the chosen node
      const uint32_t ww = (uint32_t)(__ffsll((long long)wm) - 1);
      out.ap = sh_.asm_ap[pb][ww]; out.rp = sh_.asm_rp[pb][ww]; out.fitbits = sh_.asm_fit[pb][ww];
    }
    if (threadIdx.x == 0) sh_.hit_w[hp] = BS_INF;             // (re-armed behind the barrier; the NEXT search uses the other word)
    BS_SEQ_P(12);
    if (found != BS_INF && owner && mine == found) {
      // ---- assume (NodeInfo.AddPod): requested += request, pods lane + 1; the left arrays and the meta word follow
      const uint32_t at = found;
      uint32_t nrp = rp;
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        if (j < L) {
          int64_t nr = rq[j];
          bool touched = false;
          if (j < 3) { nr = wadd(rq[j], q.preq[j]); touched = true; }
          else if (j == 3) { nr = wadd(rq[j], 1); touched = true; }
          else if ((q.ppres >> (j - 4)) & 1u) {
            nr = wadd(((rp >> (j - 4)) & 1u) ? rq[j] : 0, q.preq[j]);
            nrp |= 1u << (j - 4);
            touched = true;
          }
          if (touched) {
            sq.nreq[(size_t)j * nd.stride + at] = nr;
            if (j < 4 || ((rp >> (j - 4)) & 1u)) {             // left = scaled allocatable - requested: it moves by what requested moves by
              const int64_t dlt = wsub(nr, rq[j]);
              sq.left07[(size_t)j * nd.stride + at] = wsub(l07[j], dlt);
              sq.left10[(size_t)j * nd.stride + at] = wsub(l10[j], dlt);
            } else {                                           // a scalar key the node's requests did not have: the lane starts to exist
              sq.left07[(size_t)j * nd.stride + at] = wsub(scale_f32(al[j], 0.7f), nr);
              sq.left10[(size_t)j * nd.stride + at] = wsub(scale_f32(al[j], 1.0f), nr);
            }
          }
        }
      }
      if (nrp != rp) {
        sq.rpres[at] = nrp;
        sq.nmeta[at] = (meta & 0xFu) | ((ap & nrp) << 4);
      }
      if (prm.prune) {                                       // a negative request frees capacity: the bounds must stay upper bounds
        const int64_t n0 = wsub(al[0], wadd(rq[0], q.preq[0])), n1 = wsub(al[1], wadd(rq[1], q.preq[1]));
        if (n0 > sh_.pmax[0][at >> 6]) sh_.pmax[0][at >> 6] = n0;
        if (n1 > sh_.pmax[1][at >> 6]) sh_.pmax[1][at >> 6] = n1;
        if (seq_joint(n0, n1) > sh_.pmax[2][at >> 6]) sh_.pmax[2][at >> 6] = seq_joint(n0, n1);
        atomicAnd(&sh_.tight[at >> 11], ~(1u << ((at >> 6) & 31u)));     // the node that held a maximum may be the one that just filled up
      }
    }
  }
  BS_SEQ_P(13);
  return found;
}

// ---------------------------------------------------------------------------------------------------------------------
// The scored node choice + the assume step (rule P; bs_seq_run_scored).  seq_pick's tile walk — thread t votes for tile chunk + t, wave w
// visits its 64 tiles of a chunk with a lane per node — as a FULL search: no early stop, no cursor, no start tile.  The per-tile bounds
// still skip tiles (a tile they exclude holds no candidate: neither the maximum nor the count can change).  The fit test is seq_pick's
// flag-less one, word for word.  Every lane keeps the best candidate it has seen over all its wave's tiles as a 64-bit key
// total << 32 | (0xFFFFFFFF - node) — the largest total, then the lowest index — and, beside it, that node's values as the assume step needs
// them; keys are reduced over the wave, then over the waves through LDS (one barrier), and the lane that owns the winner assumes from its
// own registers.  Returns the node (BS_INF none), wave-uniform, identical in every wave; total_out / nfit_out likewise.
// The assume step is seq_pick's, restated on the kept values (a shared function would change seq_pick's instructions).
// ---------------------------------------------------------------------------------------------------------------------
// Under NOM (rule SP; bs_seq_run_scored_nominated) the fit test is rule S's: a node with a row chain adds the live rows the pod sees to its
// requests, exactly as seq_pick<TS, true> does, and nothing else moves — the key and score_total are fed the RAW al / rq (D8: no row enters
// a score).  The lean form does not keep the row sums: it walks the chain once per lane the pod asks for, tests, and discards.
template <int TS, bool NOM = false>
__device__ __forceinline__ uint32_t seq_pick_scored(const NodesDev& nd, const SeqDev& sq, const SeqParams& prm, SeqShared& sh_, SeqScoreShared& ss, const SeqPick& q,
                                                    const SeqScore& sco, const uint32_t (&slot_key)[kSeqCacheSlots], bool drained, SeqAssumed& out,
                                                    unsigned long long& tiles_looked, uint32_t& total_out, uint32_t& nfit_out, uint32_t pw,
                                                    const SeqPickNom& pn = SeqPickNom{}) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), S = sh.S();
  // The instantiations for more than kSeqScoredFullLanes scalar lanes are built LEAN, so that they need no scratch memory: such a search
  // keeps the key and the node's words only and the winning lane fetches its node's lanes behind the decision (one lane, one trip), and it
  // reads the pod's scalar request lanes from the staged window in LDS (pw) where it needs them instead of holding up to twelve more
  // wave-uniform int64 (q.preq[4..] is not filled for it).
  constexpr bool kLean = TS > kSeqScoredFullLanes;
  auto preq_s = [&](uint32_t j) -> int64_t {
    if constexpr (kLean) return sh_.pw_req[j][pw]; else return q.preq[j];
  };
  const int lane = lane_id(), w = (int)uni32((uint32_t)wave_id());
  const uint32_t N = nd.n;
  out.ap = out.rp = out.fitbits = 0;
  total_out = 0;
  nfit_out = 0;
  if (!drained) __syncthreads();                                            // the assume steps of earlier pods have landed before a tile is read
  if (!N || q.pcls >= nd.n_classes || q.fl >= 16u) return BS_INF;          // (ERR_PG_NOT_FOUND / the nil-leader panic: Filter fails everywhere)
  const bool fl_all = q.fl != BS_FL_EVALUATED;                              // Filter passes on every node
  const uint32_t ntiles = (N + 63u) >> 6;
  const uint32_t* fitrow = nd.fit + (size_t)q.pcls * nd.fit_words;
  unsigned long long best = 0ull;                                           // this lane's best candidate and its node's values
  int64_t b_al[BS_MAX_LANES], b_rq[BS_MAX_LANES], b_l07[BS_MAX_LANES], b_l10[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { b_al[j] = 0; b_rq[j] = 0; b_l07[j] = 0; b_l10[j] = 0; }
  uint32_t b_ap = 0, b_rp = 0, b_fbits = 0, b_meta = 0;
  uint32_t cnt = 0;                                                         // candidates this wave has seen (wave-uniform)
  for (uint32_t chunk = 0; chunk < ntiles; chunk += kSeqBlock) {
    const uint32_t t = chunk + threadIdx.x;
    bool cand = t < ntiles;
    if (cand && prm.prune) {
      cand = !(q.preq[0] > 0 && sh_.pmax[0][t] < q.preq[0]) && !(q.preq[1] > 0 && sh_.pmax[1][t] < q.preq[1]);
      if (q.preq[0] > 0 && q.preq[1] > 0) cand = cand && !(sh_.pmax[2][t] < seq_joint(q.preq[0], q.preq[1]));
    }
    unsigned long long cm = __ballot(cand);
    while (cm) {
      const uint32_t tile = chunk + ((uint32_t)w << 6) + (uint32_t)(__ffsll((long long)cm) - 1);
      cm &= cm - 1ull;
      tiles_looked++;
      const uint32_t n = (tile << 6) + (uint32_t)lane;
      const bool valid = n < N;
      const uint32_t nn = valid ? n : N - 1u;
      const uint32_t fl = nd.flags[nn];
      const uint32_t ap = nd.apres[nn], rp = sq.rpres[nn];
      const uint32_t fw = fitrow[nn >> 5];
      uint32_t fws[kSeqCacheSlots];
#pragma unroll
      for (uint32_t c = 0; c < kSeqCacheSlots; ++c)
        fws[c] = (c < prm.cache_slots && slot_key[c] != BS_INF) ? nd.fit[(size_t)(slot_key[c] >> 1) * nd.fit_words + (nn >> 5)] : 0u;
      int64_t al[BS_MAX_LANES], rq[BS_MAX_LANES], l07[BS_MAX_LANES], l10[BS_MAX_LANES];
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        al[j] = 0; rq[j] = 0; l07[j] = 0; l10[j] = 0;
        if (j < L) {
          al[j] = nd.alloc[(size_t)j * nd.stride + nn];
          rq[j] = sq.nreq[(size_t)j * nd.stride + nn];
          if constexpr (!kLean) {
            l07[j] = sq.left07[(size_t)j * nd.stride + nn];     // (for the assume step: no second round trip behind the decision)
            l10[j] = sq.left10[(size_t)j * nd.stride + nn];
          }
        }
      }
      const uint32_t meta = sq.nmeta[nn];
      uint32_t fbits = 0;
#pragma unroll
      for (uint32_t c = 0; c < kSeqCacheSlots; ++c) fbits |= ((fws[c] >> (nn & 31u)) & 1u) << c;
      const bool sched = valid && fl == 0u;
      bool ok = sched && ((fw >> (nn & 31u)) & 1u);
      const int64_t f0 = wsub(al[0], rq[0]), f1 = wsub(al[1], rq[1]);
      if (!fl_all) {                                         // computeResourceSatisfied on this node (core.go:545-563)
        bool c2 = !(q.ff & 1u), c3h = !(q.ff & 2u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t left = wsub(al[j], rq[j]);                                                   // getLeftResource :460-463
          c2 = c2 && left >= q.FR[j];
          c3h = c3h && left >= q.FM[j];
        }
        ok = ok && (c2 || !c3h);                                                                     // case 2 | case 3
      }
      bool plain = true;                                     // the node has no row chain: the flag-less fit test
      if constexpr (NOM) {
        const uint32_t head = (valid && pn.nom->view) ? pn.nom->view->nhead[nn] : kNmNone;
        if (head != kNmNone) {                               // rule S: requests plus the live rows the pod sees (a LOCAL sum; the score below stays raw)
          plain = false;
          const NomView nm = *pn.nom->view;
          if constexpr (!kLean) {
            int64_t add[BS_MAX_LANES];
#pragma unroll
            for (uint32_t j = 0; j < BS_MAX_LANES; ++j) add[j] = 0;
            seq_nominees<TS>(nm, pn.nom->consumed, head, pn.prio, pn.own, sh, add);
#pragma unroll
            for (int j = 0; j < 3; ++j) ok = ok && !(q.preq[j] > 0 && q.preq[j] > wsub(al[j], wadd(rq[j], add[j])));
            ok = ok && !(wadd(wadd(rq[3], add[3]), 1) > al[3]);
#pragma unroll
            for (uint32_t s = 0; s < BS_MAX_SCALARS; ++s) {
              if (s < S && ((q.ppres >> s) & 1u) && q.preq[4 + s] > 0) {
                const int64_t r0 = wadd(((rp >> s) & 1u) ? rq[4 + s] : 0, add[4 + s]);
                ok = ok && ((ap >> s) & 1u) && !(q.preq[4 + s] > wsub(al[4 + s], r0));
              }
            }
          } else {
            // one walk of the chain per lane the pod asks for (the pods lane always): chains are short and rows are rare
#pragma unroll
            for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
              if (j < L) {
                const int64_t pr = j < 4 ? q.preq[j] : preq_s(j);
                const bool asks = j == 3 || (pr > 0 && (j < 3 || ((q.ppres >> (j - 4)) & 1u)));
                if (asks) {
                  const int64_t add = seq_nominees_lane(nm, pn.nom->consumed, head, pn.prio, pn.own, j);
                  if (j < 3) ok = ok && !(pr > wsub(al[j], wadd(rq[j], add)));
                  else if (j == 3) ok = ok && !(wadd(wadd(rq[3], add), 1) > al[3]);
                  else {
                    const int64_t r0 = wadd(((rp >> (j - 4)) & 1u) ? rq[j] : 0, add);
                    ok = ok && ((ap >> (j - 4)) & 1u) && !(pr > wsub(al[j], r0));
                  }
                }
              }
            }
          }
        }
      }
      if (plain) {
#pragma unroll
      for (int j = 0; j < 3; ++j) ok = ok && !(q.preq[j] > 0 && q.preq[j] > wsub(al[j], rq[j]));
      ok = ok && !(wadd(rq[3], 1) > al[3]);
#pragma unroll
      for (uint32_t s = 0; s < BS_MAX_SCALARS; ++s) {
        if (s < S && ((q.ppres >> s) & 1u) && preq_s(4 + s) > 0) {
          const int64_t r0 = ((rp >> s) & 1u) ? rq[4 + s] : 0;
          ok = ok && ((ap >> s) & 1u) && !(preq_s(4 + s) > wsub(al[4 + s], r0));
        }
      }
      }
      if (ok) {                                              // rule P: R = requested + request (wrapping), cpu and memory only
        const uint32_t total = score_total(al[0], score_wadd(rq[0], q.preq[0]), al[1], score_wadd(rq[1], q.preq[1]), sco.w_least, sco.w_most, sco.w_balanced);
        const unsigned long long key = ((unsigned long long)total << 32) | (unsigned long long)(0xFFFFFFFFu - n);
        if (key > best) {
          best = key;
          if constexpr (!kLean) {
#pragma unroll
            for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { b_al[j] = al[j]; b_rq[j] = rq[j]; b_l07[j] = l07[j]; b_l10[j] = l10[j]; }
          }
          b_ap = ap; b_rp = rp; b_fbits = fbits; b_meta = meta;
        }
      }
      const unsigned long long m = __ballot(ok);
      cnt += (uint32_t)__popcll(m);
      if (!m && prm.prune && !((sh_.tight[tile >> 5] >> (tile & 31u)) & 1u)) {   // looked at in vain: tighten the tile's bounds to what is really there
        const long long m0 = readlane63_i64(wave_max_i64_lane63(sched ? (long long)f0 : INT64_MIN));
        const long long m1 = readlane63_i64(wave_max_i64_lane63(sched ? (long long)f1 : INT64_MIN));
        const long long m2 = readlane63_i64(wave_max_i64_lane63(sched ? seq_joint(f0, f1) : INT64_MIN));
        if constexpr (NOM) {                                 // (not a wild tile's: its bounds stay open, see the prologue of the pass)
          if (lane == 0 && !((pn.ns->wild[tile >> 5] >> (tile & 31u)) & 1u)) { sh_.pmax[0][tile] = m0; sh_.pmax[1][tile] = m1; sh_.pmax[2][tile] = m2; atomicOr(&sh_.tight[tile >> 5], 1u << (tile & 31u)); }
        } else {
        if (lane == 0) { sh_.pmax[0][tile] = m0; sh_.pmax[1][tile] = m1; sh_.pmax[2][tile] = m2; atomicOr(&sh_.tight[tile >> 5], 1u << (tile & 31u)); }
        }
      }
    }
  }
  // ---- the wave's best (one lane owns it: the node is part of the key), then the block's
  const unsigned long long wbest = wave_max_u64_all(best);
  const bool owner = best != 0ull && best == wbest;
  if (owner) { ss.key[w] = best; sh_.asm_ap[0][w] = b_ap; sh_.asm_rp[0][w] = b_rp; sh_.asm_fit[0][w] = b_fbits; }
  if (lane == 0) { if (wbest == 0ull) ss.key[w] = 0ull; ss.nfit[w] = cnt; }
  lds_barrier();
  unsigned long long top = 0ull;
  uint32_t ww = 0, nf = 0;
#pragma unroll
  for (int x = 0; x < kSeqWaves; ++x) {
    const unsigned long long k = ss.key[x];
    if (k > top) { top = k; ww = (uint32_t)x; }
    nf += ss.nfit[x];
  }
  top = uni64(top);
  ww = uni32(ww);
  nfit_out = uni32(nf);
  if (top == 0ull) return BS_INF;
  const uint32_t found = 0xFFFFFFFFu - (uint32_t)top;
  total_out = (uint32_t)(top >> 32);
  out.ap = sh_.asm_ap[0][ww]; out.rp = sh_.asm_rp[0][ww]; out.fitbits = sh_.asm_fit[0][ww];
  if (owner && best == top) {
    // ---- assume (NodeInfo.AddPod): requested += request, pods lane + 1; the left arrays and the meta word follow
    const uint32_t at = found;
    if constexpr (kLean) {
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        if (j < L) {
          b_al[j] = nd.alloc[(size_t)j * nd.stride + at];
          b_rq[j] = sq.nreq[(size_t)j * nd.stride + at];
          b_l07[j] = sq.left07[(size_t)j * nd.stride + at];
          b_l10[j] = sq.left10[(size_t)j * nd.stride + at];
        }
      }
    }
    uint32_t nrp = b_rp;
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
      if (j < L) {
        int64_t nr = b_rq[j];
        bool touched = false;
        if (j < 3) { nr = wadd(b_rq[j], q.preq[j]); touched = true; }
        else if (j == 3) { nr = wadd(b_rq[j], 1); touched = true; }
        else if ((q.ppres >> (j - 4)) & 1u) {
          nr = wadd(((b_rp >> (j - 4)) & 1u) ? b_rq[j] : 0, preq_s(j));
          nrp |= 1u << (j - 4);
          touched = true;
        }
        if (touched) {
          sq.nreq[(size_t)j * nd.stride + at] = nr;
          if (j < 4 || ((b_rp >> (j - 4)) & 1u)) {             // left = scaled allocatable - requested: it moves by what requested moves by
            const int64_t dlt = wsub(nr, b_rq[j]);
            sq.left07[(size_t)j * nd.stride + at] = wsub(b_l07[j], dlt);
            sq.left10[(size_t)j * nd.stride + at] = wsub(b_l10[j], dlt);
          } else {                                             // a scalar key the node's requests did not have: the lane starts to exist
            sq.left07[(size_t)j * nd.stride + at] = wsub(scale_f32(b_al[j], 0.7f), nr);
            sq.left10[(size_t)j * nd.stride + at] = wsub(scale_f32(b_al[j], 1.0f), nr);
          }
        }
      }
    }
    if (nrp != b_rp) {
      sq.rpres[at] = nrp;
      sq.nmeta[at] = (b_meta & 0xFu) | ((b_ap & nrp) << 4);
    }
    if (prm.prune) {                                       // a negative request frees capacity: the bounds must stay upper bounds
      const int64_t n0 = wsub(b_al[0], wadd(b_rq[0], q.preq[0])), n1 = wsub(b_al[1], wadd(b_rq[1], q.preq[1]));
      if (n0 > sh_.pmax[0][at >> 6]) sh_.pmax[0][at >> 6] = n0;
      if (n1 > sh_.pmax[1][at >> 6]) sh_.pmax[1][at >> 6] = n1;
      if (seq_joint(n0, n1) > sh_.pmax[2][at >> 6]) sh_.pmax[2][at >> 6] = seq_joint(n0, n1);
      atomicAnd(&sh_.tight[at >> 11], ~(1u << ((at >> 6) & 31u)));     // the node that held a maximum may be the one that just filled up
    }
  }
  return found;
}

// ---------------------------------------------------------------------------------------------------------------------
// The sampled node choice + the assume step (rule F; bs_seq_run_scored_sampled, and under NOM bs_seq_run_scored_nominated_sampled).
// Upstream's findNodesThatFit does not look at every node: it walks the list from a cursor that rotates from pod to pod and stops once it has
// K feasible nodes.  seq_pick_scored deals 64 tiles of a chunk to each wave and never stops; this is an ORDERED walk with a block-uniform
// early stop.  The walk goes over SLOTS of 64 lanes in visit order: slot u is tile (t_s + u) mod ntiles, t_s the tile that holds the cursor
// s; when s is not a tile's first node that tile has two slots — slot 0 with the lanes from s & 63 on, and one more slot behind the
// last tile with the lanes in front of it.  Inside a slot the lane order is the visit order, from slot to slot the visit position grows.
// A ROUND is kSeqWaves consecutive slots, wave w takes slot kSeqWaves * r + w.  Per round every wave tests its tile (seq_pick_scored's fit
// test, word for word, the lean form included), publishes the number of members it found (SeqSampleShared::cnt, double-buffered by round
// parity), and behind ONE lds_barrier every wave forms, from the same kSeqWaves words, the members in front of its own slot and the round's
// total.  A lane keeps its candidate only if its rank (1-based, in visit order) is at most K.  The walk stops in the round whose total
// takes the count past K: the wave whose slot holds the (K+1)-th member finds its lane (the r-th set bit of its ballot) and publishes that
// member's visit position V; without a stop V = N.  The stop is decided by every wave from the same LDS words behind the same barrier, so
// every wave runs the same number of rounds and reaches every barrier.  The per-tile bounds still skip tiles — a tile they exclude holds no
// member, so neither the kept set nor V moves —, and a tile looked at in vain is tightened only when all of it was visited.
// The key is total << 32 | (0xFFFFFFFF - visit position): the largest total, then the smallest visit position; the reduction and the assume
// step are seq_pick_scored's.  Returns the node (BS_INF none), wave-uniform, identical in every wave; total_out, nfit_out (= |C'|) and
// visited_out (= V) likewise.  With K = N and s = 0 the visit position is the node index and nothing stops: the choice is seq_pick_scored's.
// ---------------------------------------------------------------------------------------------------------------------
template <int TS, bool NOM>
__device__ __forceinline__ uint32_t seq_pick_sampled(const NodesDev& nd, const SeqDev& sq, const SeqParams& prm, SeqShared& sh_, SeqScoreShared& ss, SeqSampleShared& sm,
                                                     const SeqPick& q, const SeqScore& sco, uint32_t K, uint32_t s, const uint32_t (&slot_key)[kSeqCacheSlots],
                                                     bool drained, SeqAssumed& out, unsigned long long& tiles_looked, uint32_t& total_out, uint32_t& nfit_out,
                                                     uint32_t& visited_out, uint32_t pw, const SeqPickNom& pn) {
  const Shape<TS> sh(prm.S);
  const uint32_t L = sh.L(), S = sh.S();
  constexpr bool kLean = TS > kSeqScoredFullLanes;           // (see seq_pick_scored)
  auto preq_s = [&](uint32_t j) -> int64_t {
    if constexpr (kLean) return sh_.pw_req[j][pw]; else return q.preq[j];
  };
  const int lane = lane_id(), w = (int)uni32((uint32_t)wave_id());
  const uint32_t N = nd.n;
  out.ap = out.rp = out.fitbits = 0;
  total_out = 0;
  nfit_out = 0;
  visited_out = N;                                                          // no stop, and the two early exits below: C is empty, the walk saw every node
  if (!drained) __syncthreads();                                            // the assume steps of earlier pods have landed before a tile is read
  if (!N || q.pcls >= nd.n_classes || q.fl >= 16u) return BS_INF;          // (ERR_PG_NOT_FOUND / the nil-leader panic: Filter fails everywhere)
  const bool fl_all = q.fl != BS_FL_EVALUATED;                              // Filter passes on every node
  const uint32_t ntiles = (N + 63u) >> 6;
  const uint32_t* fitrow = nd.fit + (size_t)q.pcls * nd.fit_words;
  const uint32_t ts = s >> 6, off = s & 63u;                                // the cursor's tile and lane
  const uint32_t slots = ntiles + (off ? 1u : 0u), rounds = (slots + (uint32_t)kSeqWaves - 1u) / (uint32_t)kSeqWaves;
  unsigned long long best = 0ull;                                           // this lane's best KEPT candidate and its node's values
  int64_t b_al[BS_MAX_LANES], b_rq[BS_MAX_LANES], b_l07[BS_MAX_LANES], b_l10[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { b_al[j] = 0; b_rq[j] = 0; b_l07[j] = 0; b_l10[j] = 0; }
  uint32_t b_ap = 0, b_rp = 0, b_fbits = 0, b_meta = 0;
  uint32_t base = 0;                                                        // members of C in front of the round (block-uniform)
  bool stop = false;                                                        // the (K+1)-th member has been met (block-uniform)
  for (uint32_t r = 0; r < rounds && !stop; ++r) {
    const uint32_t b = r & 1u;
    const uint32_t u = r * (uint32_t)kSeqWaves + (uint32_t)w;               // this wave's slot
    const bool in_walk = u < slots;
    uint32_t tile = in_walk ? ts + u : 0u;
    if (tile >= ntiles) tile -= ntiles;                                     // (u <= ntiles, ts < ntiles: one subtraction)
    const bool head = off != 0u && u == 0u, tail = u == ntiles;             // the two visits of the cursor's tile (a tail slot exists only with off != 0)
    bool cand = in_walk;
    if (cand && prm.prune) {
      cand = !(q.preq[0] > 0 && sh_.pmax[0][tile] < q.preq[0]) && !(q.preq[1] > 0 && sh_.pmax[1][tile] < q.preq[1]);
      if (q.preq[0] > 0 && q.preq[1] > 0) cand = cand && !(sh_.pmax[2][tile] < seq_joint(q.preq[0], q.preq[1]));
    }
    cand = __ballot(cand) != 0ull;                                          // (wave-uniform by construction; said to the compiler)
    bool ok = false;
    uint32_t n = 0, ap = 0, rp = 0, fbits = 0, meta = 0;
    int64_t al[BS_MAX_LANES], rq[BS_MAX_LANES], l07[BS_MAX_LANES], l10[BS_MAX_LANES];
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { al[j] = 0; rq[j] = 0; l07[j] = 0; l10[j] = 0; }
    unsigned long long m = 0ull;
    if (cand) {
      tiles_looked++;
      n = (tile << 6) + (uint32_t)lane;
      const bool valid = n < N;
      const uint32_t nn = valid ? n : N - 1u;
      const uint32_t fl = nd.flags[nn];
      ap = nd.apres[nn];
      rp = sq.rpres[nn];
      const uint32_t fw = fitrow[nn >> 5];
      uint32_t fws[kSeqCacheSlots];
#pragma unroll
      for (uint32_t c = 0; c < kSeqCacheSlots; ++c)
        fws[c] = (c < prm.cache_slots && slot_key[c] != BS_INF) ? nd.fit[(size_t)(slot_key[c] >> 1) * nd.fit_words + (nn >> 5)] : 0u;
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        if (j < L) {
          al[j] = nd.alloc[(size_t)j * nd.stride + nn];
          rq[j] = sq.nreq[(size_t)j * nd.stride + nn];
          if constexpr (!kLean) {
            l07[j] = sq.left07[(size_t)j * nd.stride + nn];     // (for the assume step: no second round trip behind the decision)
            l10[j] = sq.left10[(size_t)j * nd.stride + nn];
          }
        }
      }
      meta = sq.nmeta[nn];
#pragma unroll
      for (uint32_t c = 0; c < kSeqCacheSlots; ++c) fbits |= ((fws[c] >> (nn & 31u)) & 1u) << c;
      const bool sched = valid && fl == 0u;
      ok = sched && ((fw >> (nn & 31u)) & 1u);
      const int64_t f0 = wsub(al[0], rq[0]), f1 = wsub(al[1], rq[1]);
      if (!fl_all) {                                         // computeResourceSatisfied on this node (core.go:545-563)
        bool c2 = !(q.ff & 1u), c3h = !(q.ff & 2u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t left = wsub(al[j], rq[j]);                                                   // getLeftResource :460-463
          c2 = c2 && left >= q.FR[j];
          c3h = c3h && left >= q.FM[j];
        }
        ok = ok && (c2 || !c3h);                                                                     // case 2 | case 3
      }
      bool plain = true;                                     // the node has no row chain: the flag-less fit test
      if constexpr (NOM) {
        const uint32_t head_r = (valid && pn.nom->view) ? pn.nom->view->nhead[nn] : kNmNone;
        if (head_r != kNmNone) {                             // rule S: requests plus the live rows the pod sees (a LOCAL sum; the score below stays raw)
          plain = false;
          const NomView nm = *pn.nom->view;
          if constexpr (!kLean) {
            int64_t add[BS_MAX_LANES];
#pragma unroll
            for (uint32_t j = 0; j < BS_MAX_LANES; ++j) add[j] = 0;
            seq_nominees<TS>(nm, pn.nom->consumed, head_r, pn.prio, pn.own, sh, add);
#pragma unroll
            for (int j = 0; j < 3; ++j) ok = ok && !(q.preq[j] > 0 && q.preq[j] > wsub(al[j], wadd(rq[j], add[j])));
            ok = ok && !(wadd(wadd(rq[3], add[3]), 1) > al[3]);
#pragma unroll
            for (uint32_t s2 = 0; s2 < BS_MAX_SCALARS; ++s2) {
              if (s2 < S && ((q.ppres >> s2) & 1u) && q.preq[4 + s2] > 0) {
                const int64_t r0 = wadd(((rp >> s2) & 1u) ? rq[4 + s2] : 0, add[4 + s2]);
                ok = ok && ((ap >> s2) & 1u) && !(q.preq[4 + s2] > wsub(al[4 + s2], r0));
              }
            }
          } else {
            // one walk of the chain per lane the pod asks for (the pods lane always): chains are short and rows are rare
#pragma unroll
            for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
              if (j < L) {
                const int64_t pr = j < 4 ? q.preq[j] : preq_s(j);
                const bool asks = j == 3 || (pr > 0 && (j < 3 || ((q.ppres >> (j - 4)) & 1u)));
                if (asks) {
                  const int64_t add = seq_nominees_lane(nm, pn.nom->consumed, head_r, pn.prio, pn.own, j);
                  if (j < 3) ok = ok && !(pr > wsub(al[j], wadd(rq[j], add)));
                  else if (j == 3) ok = ok && !(wadd(wadd(rq[3], add), 1) > al[3]);
                  else {
                    const int64_t r0 = wadd(((rp >> (j - 4)) & 1u) ? rq[j] : 0, add);
                    ok = ok && ((ap >> (j - 4)) & 1u) && !(pr > wsub(al[j], r0));
                  }
                }
              }
            }
          }
        }
      }
      if (plain) {
#pragma unroll
      for (int j = 0; j < 3; ++j) ok = ok && !(q.preq[j] > 0 && q.preq[j] > wsub(al[j], rq[j]));
      ok = ok && !(wadd(rq[3], 1) > al[3]);
#pragma unroll
      for (uint32_t s2 = 0; s2 < BS_MAX_SCALARS; ++s2) {
        if (s2 < S && ((q.ppres >> s2) & 1u) && preq_s(4 + s2) > 0) {
          const int64_t r0 = ((rp >> s2) & 1u) ? rq[4 + s2] : 0;
          ok = ok && ((ap >> s2) & 1u) && !(preq_s(4 + s2) > wsub(al[4 + s2], r0));
        }
      }
      }
      const unsigned long long all = __ballot(ok);           // over every valid lane of the tile: what "looked at in vain" means
      if (head) ok = ok && (uint32_t)lane >= off;            // the cursor's tile, first visit: the lanes from the cursor on
      if (tail) ok = ok && (uint32_t)lane < off;             // ... and its second, at the end of the walk: the lanes in front of it
      m = __ballot(ok);
      if (!all && !head && !tail && prm.prune && !((sh_.tight[tile >> 5] >> (tile & 31u)) & 1u)) {   // looked at in vain: tighten the tile's bounds to what is really there
        const long long m0 = readlane63_i64(wave_max_i64_lane63(sched ? (long long)f0 : INT64_MIN));
        const long long m1 = readlane63_i64(wave_max_i64_lane63(sched ? (long long)f1 : INT64_MIN));
        const long long m2 = readlane63_i64(wave_max_i64_lane63(sched ? seq_joint(f0, f1) : INT64_MIN));
        if constexpr (NOM) {                                 // (not a wild tile's: its bounds stay open, see the prologue of the pass)
          if (lane == 0 && !((pn.ns->wild[tile >> 5] >> (tile & 31u)) & 1u)) { sh_.pmax[0][tile] = m0; sh_.pmax[1][tile] = m1; sh_.pmax[2][tile] = m2; atomicOr(&sh_.tight[tile >> 5], 1u << (tile & 31u)); }
        } else {
          if (lane == 0) { sh_.pmax[0][tile] = m0; sh_.pmax[1][tile] = m1; sh_.pmax[2][tile] = m2; atomicOr(&sh_.tight[tile >> 5], 1u << (tile & 31u)); }
        }
      }
    }
    // ---- the count exchange: the members in front of this wave's slot, and the round's total
    const uint32_t cw = sample_popc64(m);
    if (lane == 0) sm.cnt[b][w] = cw;
    lds_barrier();
    uint32_t before = base, round_total = 0;
#pragma unroll
    for (int x = 0; x < kSeqWaves; ++x) {
      const uint32_t c = sm.cnt[b][x];
      if (x < w) before += c;
      round_total += c;
    }
    before = uni32(before);
    round_total = uni32(round_total);
    if (ok) {                                                // rule F: the first K members in visit order are kept, the rest is not
      const uint32_t rank = before + sample_popc64(m & ((1ull << lane) - 1ull)) + 1u;
      if (rank <= K) {                                       // rule P on the kept: R = requested + request (wrapping), cpu and memory only
        const uint32_t total = score_total(al[0], score_wadd(rq[0], q.preq[0]), al[1], score_wadd(rq[1], q.preq[1]), sco.w_least, sco.w_most, sco.w_balanced);
        const unsigned long long key = ((unsigned long long)total << 32) | (unsigned long long)(0xFFFFFFFFu - sample_pos(s, n, N));
        if (key > best) {
          best = key;
          if constexpr (!kLean) {
#pragma unroll
            for (uint32_t j = 0; j < BS_MAX_LANES; ++j) { b_al[j] = al[j]; b_rq[j] = rq[j]; b_l07[j] = l07[j]; b_l10[j] = l10[j]; }
          }
          b_ap = ap; b_rp = rp; b_fbits = fbits; b_meta = meta;
        }
      }
    }
    // ---- the stop: the same words, the same arithmetic, in every wave
    stop = round_total > K - base;                           // (base <= K while the walk goes on)
    if (stop && before <= K && K - before < cw) {            // this wave's slot holds the (K+1)-th member: it is not kept, the walk ends in front of it
      const uint32_t ln = sample_nth_bit(m, K - before + 1u);
      if (lane == 0) sm.vstop = sample_pos(s, (tile << 6) + ln, N);
    }
    base += round_total;
  }
  // ---- the wave's best (one lane owns it: the visit position is part of the key), then the block's
  const unsigned long long wbest = wave_max_u64_all(best);
  const bool owner = best != 0ull && best == wbest;
  if (owner) { ss.key[w] = best; sh_.asm_ap[0][w] = b_ap; sh_.asm_rp[0][w] = b_rp; sh_.asm_fit[0][w] = b_fbits; }
  if (lane == 0 && wbest == 0ull) ss.key[w] = 0ull;
  lds_barrier();
  unsigned long long top = 0ull;
  uint32_t ww = 0;
#pragma unroll
  for (int x = 0; x < kSeqWaves; ++x) {
    const unsigned long long k = ss.key[x];
    if (k > top) { top = k; ww = (uint32_t)x; }
  }
  top = uni64(top);
  ww = uni32(ww);
  nfit_out = stop ? K : base;
  if (stop) visited_out = uni32(sm.vstop);
  if (top == 0ull) return BS_INF;
  const uint32_t found = sample_node(s, 0xFFFFFFFFu - (uint32_t)top, N);
  total_out = (uint32_t)(top >> 32);
  out.ap = sh_.asm_ap[0][ww]; out.rp = sh_.asm_rp[0][ww]; out.fitbits = sh_.asm_fit[0][ww];
  if (owner && best == top) {
    // ---- assume (NodeInfo.AddPod): requested += request, pods lane + 1; the left arrays and the meta word follow
    const uint32_t at = found;
    if constexpr (kLean) {
#pragma unroll
      for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
        if (j < L) {
          b_al[j] = nd.alloc[(size_t)j * nd.stride + at];
          b_rq[j] = sq.nreq[(size_t)j * nd.stride + at];
          b_l07[j] = sq.left07[(size_t)j * nd.stride + at];
          b_l10[j] = sq.left10[(size_t)j * nd.stride + at];
        }
      }
    }
    uint32_t nrp = b_rp;
#pragma unroll
    for (uint32_t j = 0; j < BS_MAX_LANES; ++j) {
      if (j < L) {
        int64_t nr = b_rq[j];
        bool touched = false;
        if (j < 3) { nr = wadd(b_rq[j], q.preq[j]); touched = true; }
        else if (j == 3) { nr = wadd(b_rq[j], 1); touched = true; }
        else if ((q.ppres >> (j - 4)) & 1u) {
          nr = wadd(((b_rp >> (j - 4)) & 1u) ? b_rq[j] : 0, preq_s(j));
          nrp |= 1u << (j - 4);
          touched = true;
        }
        if (touched) {
          sq.nreq[(size_t)j * nd.stride + at] = nr;
          if (j < 4 || ((b_rp >> (j - 4)) & 1u)) {             // left = scaled allocatable - requested: it moves by what requested moves by
            const int64_t dlt = wsub(nr, b_rq[j]);
            sq.left07[(size_t)j * nd.stride + at] = wsub(b_l07[j], dlt);
            sq.left10[(size_t)j * nd.stride + at] = wsub(b_l10[j], dlt);
          } else {                                             // a scalar key the node's requests did not have: the lane starts to exist
            sq.left07[(size_t)j * nd.stride + at] = wsub(scale_f32(b_al[j], 0.7f), nr);
            sq.left10[(size_t)j * nd.stride + at] = wsub(scale_f32(b_al[j], 1.0f), nr);
          }
        }
      }
    }
    if (nrp != b_rp) {
      sq.rpres[at] = nrp;
      sq.nmeta[at] = (b_meta & 0xFu) | ((b_ap & nrp) << 4);
    }
    if (prm.prune) {                                       // a negative request frees capacity: the bounds must stay upper bounds
      const int64_t n0 = wsub(b_al[0], wadd(b_rq[0], q.preq[0])), n1 = wsub(b_al[1], wadd(b_rq[1], q.preq[1]));
      if (n0 > sh_.pmax[0][at >> 6]) sh_.pmax[0][at >> 6] = n0;
      if (n1 > sh_.pmax[1][at >> 6]) sh_.pmax[1][at >> 6] = n1;
      if (seq_joint(n0, n1) > sh_.pmax[2][at >> 6]) sh_.pmax[2][at >> 6] = seq_joint(n0, n1);
      atomicAnd(&sh_.tight[at >> 11], ~(1u << ((at >> 6) & 31u)));     // the node that held a maximum may be the one that just filled up
    }
  }
  return found;
}

// findMaxPG (core.go:701-739) over the keys.  Wave-uniform result: leader (-1 none), panic.
__device__ __forceinline__ void seq_find_max(const GroupsDev& gr, const SeqDev& sq, const SeqParams& prm, SeqShared& sh_, const unsigned long long* lkeys,
                                             int32_t& leader, bool& panic, unsigned long long& top_out) {
  const uint32_t G = gr.g;
  top_out = 0;
  auto key_at = [&](uint32_t g) -> unsigned long long {
    return prm.keys_in_lds ? lkeys[g] : __hip_atomic_load(&sq.keys[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  if (!prm.keys_in_lds) BS_SEQ_FULL_BARRIER();                      // keys in global memory: thread 0's stores of earlier pods have landed
  unsigned long long best = 0;
  for (uint32_t g = threadIdx.x; g < G; g += kSeqBlock) {
    const unsigned long long k = key_at(g);
    best = k > best ? k : best;
  }
  best = wave_max_u64_all(best);
  if (lane_id() == 0) sh_.kmax[wave_id()] = best;
  BS_SEQ_FULL_BARRIER();
  unsigned long long top = 0;
#pragma unroll
  for (int ww = 0; ww < kSeqWaves; ++ww) top = sh_.kmax[ww] > top ? sh_.kmax[ww] : top;
  top = uni64(top);
  panic = top == ~0ull;
  leader = -1;
  if (panic || top == 0ull) return;
  const uint32_t F1 = (uint32_t)(top >> 32);
  uint32_t cur = 0x7FFFFFFFu - ((uint32_t)top >> 1);
  bool full = top & 1ull;
  if (!full) top_out = top;                                  // (a fully scheduled winner may hand over: its key is no bound for the others)
  while (full) {                                             // the tie rule :729-731 may hand over (rare: exact walk)
    uint32_t nxt = BS_INF;
    for (uint32_t g = threadIdx.x; g < G; g += kSeqBlock) {
      if (g <= cur || g >= nxt) continue;
      const unsigned long long k = key_at(g);
      if (k == 0ull || (uint32_t)(k >> 32) != F1) continue;
      if (__hip_atomic_load(&sq.g_sc[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) nxt = g;
    }
    nxt = wave_min_u32(nxt);
    BS_SEQ_FULL_BARRIER();
    if (lane_id() == 0) sh_.red[wave_id()] = nxt;
    BS_SEQ_FULL_BARRIER();
    uint32_t r = BS_INF;
#pragma unroll
    for (int ww = 0; ww < kSeqWaves; ++ww) r = min(r, sh_.red[ww]);
    r = uni32(r);
    if (r == BS_INF) break;
    cur = r;
    full = uni64(key_at(cur)) & 1ull;
  }
  leader = (int32_t)cur;
}

// The input fields of pods i0 .. i0 + kSeqPodWin - 1 into LDS (the caller brackets it with barriers).  MinMember of the pod's group
// rides along (one more dependent trip per WINDOW, not per pod); nothing here is written by the pass.
template <int TS>
__device__ __forceinline__ void seq_stage_pods(const PodsDev& pods, const GroupsDev& gr, const SeqDev& sq, SeqShared& sh_, uint32_t i0, Shape<TS> sh) {
  const uint32_t P = pods.p, L = sh.L();
  for (uint32_t e = threadIdx.x; e < kSeqPodWin * L; e += kSeqBlock) {
    const uint32_t j = e / kSeqPodWin, w = e % kSeqPodWin, p = min(i0 + w, P - 1u);
    sh_.pw_req[j][w] = pods.req[(size_t)j * P + p];
  }
  if (threadIdx.x < kSeqPodWin) {
    const uint32_t w = threadIdx.x, p = min(i0 + w, P - 1u);
    const int32_t g = pods.group[p];
    sh_.pw_group[w] = g;
    sh_.pw_flags[w] = pods.flags[p];
    sh_.pw_cls[w] = pods.cls[p];
    sh_.pw_pres[w] = pods.pres[p];
    sh_.pw_owner[w] = pods.owner[p];
    sh_.pw_pclass[w] = sq.pclass ? sq.pclass[p] : 0u;
    sh_.pw_mm[w] = (g >= 0 && (uint32_t)g < gr.g) ? gr.min_member[g] : 0u;
  }
}
// getPodResourceRequire(pod) from the staged fields (pod_require's rule: the lanes normalised through Add)
template <int TS>
__device__ __forceinline__ void seq_pod_require(const SeqShared& sh_, uint32_t w, Shape<TS> sh, uint32_t gate, Res& out) {
  Res raw;
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
    if (j < sh.L()) raw.v[j] = (int64_t)uni64((uint64_t)sh_.pw_req[j][w]);
  raw.present = uni32(sh_.pw_pres[w]);
  res_zero(out, sh);
  res_add(out, raw, sh, gate);
}

// Everything the pass reads from one group, loaded in ONE round trip.  The state of the pod's own group and of the leader
// then stays in registers (wave-uniform, every wave applies the same updates): consecutive pods of a gang, and pods that
// reserve for the same leader, read nothing from global memory.
struct SeqGroup {
  uint32_t flags, matched, sc, cls, head, nwait;
  uint32_t mm;                   // Spec.MinMember (never written by the pass; fetched in the same trip)
  uint32_t seen;                 // a pod of the gang has entered PreFilter in this pass (t_first is set); a word, not a bool: no padding to copy
  uint64_t occ;
  Res mr;
};
template <int TS>
__device__ __forceinline__ void seq_group_load(const SeqDev& sq, const GroupsDev& gr, uint32_t G, uint32_t g, Shape<TS> sh, SeqGroup& o) {
  const uint32_t gmm = gr.min_member[g];
  const uint32_t f = seq_raw8(&sq.g_flags[g]), m = seq_raw32(&sq.g_matched[g]), s = seq_raw32(&sq.g_sc[g]), c = seq_raw32(&sq.g_cls[g]),
                 p = seq_raw32(&sq.g_mrpres[g]), h = seq_raw32(&sq.head[g]), nw = seq_raw32(&sq.nwait[g]);
  const uint64_t oc = seq_raw64(&sq.g_occ[g]), tf = seq_raw64(&sq.t_first[g]);
  uint64_t mr[BS_MAX_LANES];
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
    if (j < sh.L()) mr[j] = seq_raw64(&sq.g_minres[(size_t)j * G + g]);
  o.flags = uni32(f); o.matched = uni32(m); o.sc = uni32(s); o.cls = uni32(c); o.head = uni32(h); o.nwait = uni32(nw);
  o.mm = uni32(gmm);
  o.occ = uni64(oc);
  o.seen = uni64(tf) != ~0ull;
#pragma unroll
  for (uint32_t j = 0; j < BS_MAX_LANES; ++j)
    if (j < sh.L()) o.mr.v[j] = (int64_t)uni64(mr[j]);
  o.mr.present = uni32(p);
}
template <int TS>
__device__ __forceinline__ void seq_group_zero(SeqGroup& o, Shape<TS> sh) {
  o.flags = o.matched = o.sc = o.cls = o.head = o.nwait = o.mm = 0;
  o.seen = false;
  o.occ = 0;
  res_zero(o.mr, sh);
}

// The pass: its body is bs_seq_pass.inc, included by all four kernel templates.  NOM = false is bs_seq_run's kernel: six instantiations (bs_lanes.hpp,
// lanes_narrow), name and arguments as they always were.
template <int TS>
__global__ __launch_bounds__(kSeqBlock, 1) void k_seq_pass(PodsDev pods, GroupsDev gr, NodesDev nd, SeqDev sq, SeqParams prm) {
  constexpr bool NOM = false, SCORE = false, SAMPLE = false;
  const SeqNom nom{};                                        // (named by the discarded NOM-only lines)
  const SeqScore sco{};                                      // (... and by the discarded SCORE-only ones)
  const SeqSample smp{};                                     // (... and by the discarded SAMPLE-only ones)
#include "bs_seq_pass.inc"
}
// bs_seq_run_nominated's: k_seq_pass<TS, true>, rule S on top, the same six lane counts (an overload: a defaulted second parameter would
// rename the six above)
template <int TS, bool NOM>
__global__ __launch_bounds__(kSeqBlock, 1) void k_seq_pass(PodsDev pods, GroupsDev gr, NodesDev nd, SeqDev sq, SeqParams prm, SeqNom nom) {
  static_assert(NOM, "the flag-less pass is k_seq_pass<TS>");
  constexpr bool SCORE = false, SAMPLE = false;
  const SeqScore sco{};
  const SeqSample smp{};
#include "bs_seq_pass.inc"
}
// bs_seq_run_scored's: the third inclusion, rule P in the node choice (SCORE = true, NOM = false); emitted by tu_seq_score.hip.  It reads and
// writes no first-fit cursor.  One instantiation per lane count a context can have, 0 .. BS_MAX_SCALARS (bs_lanes.hpp, lanes_wide), and no
// generic-lane one: the body at TS = -1 branches on every lane of every unrolled loop and keeps more wave-uniform state than the SGPR spill
// lanes hold — 24 bytes of scratch memory before the scored search is even part of it —, and the library admits scratch in k_seq_pass alone
// (tests/test_kernel_resources.py).  With the lane count fixed, and built lean above kSeqScoredFullLanes, every instantiation is free of it.
template <int TS>
__global__ __launch_bounds__(kSeqBlock, 1) void k_seq_scored(PodsDev pods, GroupsDev gr, NodesDev nd, SeqDev sq, SeqParams prm, SeqScore sco) {
  static_assert(TS >= 0, "the scored pass has fixed-lane instantiations only");
  constexpr bool NOM = false, SCORE = true, SAMPLE = false;
  const SeqNom nom{};
  const SeqSample smp{};
#include "bs_seq_pass.inc"
}
// bs_seq_run_scored_nominated's: the fourth inclusion, rules S and P at once (rule SP: NOM = true, SCORE = true); emitted by
// tu_seq_score_nom.hip.  A name of its own (the kernel lists that count k_seq_scored and k_seq_pass by name stay what they were); the same
// thirteen lane counts as k_seq_scored, lean above kSeqScoredFullLanes, and no generic-lane one for the reason given above.
template <int TS>
__global__ __launch_bounds__(kSeqBlock, 1) void k_seq_sp(PodsDev pods, GroupsDev gr, NodesDev nd, SeqDev sq, SeqParams prm, SeqNom nom, SeqScore sco) {
  static_assert(TS >= 0, "the scored pass has fixed-lane instantiations only");
  constexpr bool NOM = true, SCORE = true, SAMPLE = false;
  const SeqSample smp{};
#include "bs_seq_pass.inc"
}
// bs_seq_run_scored_sampled's: the fifth inclusion, rule F over rule P (SCORE = true, SAMPLE = true: the node choice is seq_pick_sampled); emitted
// by tu_seq_sample.hip.  The same thirteen lane counts as k_seq_scored, lean above kSeqScoredFullLanes, no generic-lane one.  The name holds
// none of k_seq_pass, k_seq_scored, k_seq_sp: the kernel lists that count those families by name stay what they were.
template <int TS>
__global__ __launch_bounds__(kSeqBlock, 1) void k_seq_sampled(PodsDev pods, GroupsDev gr, NodesDev nd, SeqDev sq, SeqParams prm, SeqScore sco, SeqSample smp) {
  static_assert(TS >= 0, "the sampled pass has fixed-lane instantiations only");
  constexpr bool NOM = false, SCORE = true, SAMPLE = true;
  const SeqNom nom{};
#include "bs_seq_pass.inc"
}
// bs_seq_run_scored_nominated_sampled's: the sixth inclusion, rule F over rule SP (all three flags); emitted by tu_seq_sample_nom.hip
template <int TS>
__global__ __launch_bounds__(kSeqBlock, 1) void k_seq_sampled_nom(PodsDev pods, GroupsDev gr, NodesDev nd, SeqDev sq, SeqParams prm, SeqNom nom, SeqScore sco,
                                                                  SeqSample smp) {
  static_assert(TS >= 0, "the sampled pass has fixed-lane instantiations only");
  constexpr bool NOM = true, SCORE = true, SAMPLE = true;
#include "bs_seq_pass.inc"
}
// the launch of k_seq_sampled<TS> for S scalar lanes (defined in tu_seq_sample.hip; called by tu_seq.hip)
void launch_seq_sampled(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq, const SeqParams& prm,
                        const SeqScore& sco, const SeqSample& smp);
// the launch of k_seq_sampled_nom<TS> for S scalar lanes (defined in tu_seq_sample_nom.hip; called by tu_seq.hip)
void launch_seq_sampled_nominated(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq,
                                  const SeqParams& prm, const SeqNom& nom, const SeqScore& sco, const SeqSample& smp);
// the launch of k_seq_sp<TS> for S scalar lanes (defined in tu_seq_score_nom.hip; called by tu_seq.hip)
void launch_seq_scored_nominated(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq,
                                 const SeqParams& prm, const SeqNom& nom, const SeqScore& sco);
// the launch of k_seq_scored<TS> for S scalar lanes (defined in tu_seq_score.hip; called by tu_seq.hip)
void launch_seq_scored(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq, const SeqParams& prm,
                       const SeqScore& sco);
// the launch of k_seq_pass<TS, true> for S scalar lanes (defined in tu_seq_nom.hip, the unit that emits those kernels; called by tu_seq.hip)
void launch_seq_nominated(hipStream_t stream, uint32_t S, size_t lds, const PodsDev& pd, const GroupsDev& gr, const NodesDev& nd, const SeqDev& sq, const SeqParams& prm,
                          const SeqNom& nom);

}  // namespace bs
