// Layout of the batch's node words (BatchDev::nodew; written by node_words_block in bs_fast.hpp, read by the lean Filter items of bs_filter_t.hpp,
// allocated and launched by bsched.hip).  Plain C++ index arithmetic, no HIP includes: the CPU tests compile it on its own and walk every store the
// grid makes (tests/test_nodew_layout_cpu.py).  Every user calls these functions; nobody restates the arithmetic.
//
//   W      = nodew_words(N) = cdiv(N, 64)       64-node blocks, one word PAIR (ok, ~holds) each
//   stride = nodew_stride(N) = W + 2            pairs per table: the lean loop's scalar loads run ahead of the block they work on, so a table ends in
//                                               two pairs nobody writes and nobody uses
//   table t in [0, 3), block w in [0, W):       uint64 index nodew_pair(stride, t, w) and the one behind it
//   ref[]:                                      nodew_ref(stride) + 4 s + j (maxSingle of leader s, fixed lane j), + 8 + s (its flag word)
//   uint64 words to allocate:                   nodew_alloc_words(N)
//
// The grid that writes the tables has nodew_blocks(N) blocks of kNodewBlockThreads threads, thread = node, wave = 64-node block
// w = nodew_wave_word(block, thread).  N need not fill the last block: its waves with w >= W have no node at all, and nodew_wave_stores(N, w) tells
// them to store nothing — table t's pair W + 2 is table t + 1's pair 0 (and ref[0..1] behind the last table), which block 0 writes in the same launch.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BS_NODEW_HD __host__ __device__ __attribute__((always_inline)) inline      // (inlined before anything else runs: the callers compile as if the arithmetic stood in them)
#else
#define BS_NODEW_HD inline
#endif

namespace bs {

constexpr int kNodewTables = 3;                 // 0: the batch's findMaxPG result, 1: the leader carried into the batch, 2: a leader with a scalar MinResources
constexpr int kNodewLeaders = 2;                // tables 0 and 1 leave their maxSingle in ref[]
constexpr uint32_t kNodewBlockThreads = 256;    // == kTblChunk (bs_kernels.hpp checks)
constexpr uint32_t kNodewRefWords = 16;         // ref[]: 2 x 4 maxSingle lanes, 2 flag words, padding

BS_NODEW_HD constexpr uint32_t nodew_words(uint32_t n_nodes) { return (n_nodes + 63u) / 64u; }
BS_NODEW_HD constexpr uint32_t nodew_stride(uint32_t n_nodes) { return nodew_words(n_nodes) + 2u; }
// (table and leader indices are small ints, as the kernels hold them)
BS_NODEW_HD constexpr size_t nodew_table(uint32_t stride, int t) { return (size_t)t * stride * 2; }
BS_NODEW_HD constexpr size_t nodew_pair(uint32_t stride, int t, uint32_t w) { return ((size_t)t * stride + w) * 2; }
BS_NODEW_HD constexpr size_t nodew_ref(uint32_t stride) { return (size_t)(2 * kNodewTables) * stride; }
BS_NODEW_HD constexpr int nodew_ref_lane_at(int s, int j) { return 4 * s + j; }                      // relative to nodew_ref()
BS_NODEW_HD constexpr int nodew_ref_flags_at(int s) { return 4 * (int)kNodewLeaders + s; }
BS_NODEW_HD constexpr size_t nodew_ref_lane(uint32_t stride, int s, int j) { return nodew_ref(stride) + nodew_ref_lane_at(s, j); }
BS_NODEW_HD constexpr size_t nodew_ref_flags(uint32_t stride, int s) { return nodew_ref(stride) + nodew_ref_flags_at(s); }
BS_NODEW_HD constexpr size_t nodew_alloc_words(uint32_t n_nodes) { return nodew_ref(nodew_stride(n_nodes)) + kNodewRefWords; }
BS_NODEW_HD constexpr uint32_t nodew_blocks(uint32_t n_nodes) { return (n_nodes + kNodewBlockThreads - 1u) / kNodewBlockThreads; }
BS_NODEW_HD constexpr uint32_t nodew_wave_word(uint32_t block, uint32_t thread) { return (block * kNodewBlockThreads + thread) >> 6; }
BS_NODEW_HD constexpr bool nodew_wave_stores(uint32_t n_nodes, uint32_t w) { return w < nodew_words(n_nodes); }

static_assert(nodew_ref_flags_at(kNodewLeaders - 1) < (int)kNodewRefWords, "ref[] holds the leaders' maxSingle and flag words");

}  // namespace bs
