// bs_nominated.hpp — the resident nominated-pod table (include/bsched.h, bs_nominated_*): pods that preempted in an earlier cycle and have
// not bound yet.  Upstream's podFitsOnNode adds them to the node before every fit test of the victim search (addNominatedPods: the pods
// nominated on the node with priority >= the pod under test); here the three preemption calls do, by rule N of the header.
//
// The table follows the wait table's form (bs_wait.hpp): one row per nominee — id, node, priority, the request lanes as AddPod counts them
// (lanes 0..2 the request, the pods lane 1, a scalar lane the request where the present bit is set, else 0), the present bits masked to the
// context's scalar lanes — in ascending id, in one allocation with a twin.  Beside the rows: nhead[N] and nnext[cap] (kNmNone = none), one
// chain per node through the rows on it.  The order inside a chain is whatever k_nm_chains' exchanges produce: nothing depends on it, the
// sums over a chain are wrapping adds.
//
// Kernels of bs_nominated_apply, handed over by launch boundary only.  Every change goes from the live table into the twin:
//   k_nm_mark       one lane per listed id: a binary search in the id column (ascending), flag[row] = 1.  The host has checked the list
//                   against the ids it keeps (bs_nominated_check.hpp): every id is live and listed once.
//   k_nm_move<S>    ONE workgroup of 1024 threads walks the rows in windows of 1024 with a running base: a survivor's position is the base
//                   plus the survivors in front of it inside the window (a ballot inside the wave, the waves' counts through LDS).  The
//                   table holds at most BS_NOM_MAX = 65536 rows, 64 windows: no grid-wide hand-over is worth its price.  Stable.
//   k_nm_gather<S>  one thread per inserted row: id = ids + k, node and priority from the call, the request lanes and present bits from the
//                   resident queue at pod_index[k] (as k_wt_gather stores a waiting pod), appended behind the survivors.
//   k_nm_chains     one thread per row of the new table: nnext[row] = exchange(nhead[node], row) (nhead was filled with kNmNone); thread 0
//                   writes the NomView of the new table beside it.
// The table follows node-list surgery (bs_nominated_nodes_apply) by one more kernel into the twin; k_nm_chains then runs for the new count:
//   k_nn_move<S>    k_nm_move's walk with another test: the host hands over the sorted OLD nodes that leave (bs_bound_nodes_replay.hpp);
//                   every thread makes the one binary search of its row's node k in that list (lo = removed nodes below k: the row is gone
//                   when rem[lo] == k, else its node becomes k - lo).  A survivor goes to base + rank with the new node; a dropped row
//                   goes to output row e - (survivors in front of it) as (id, OLD node, priority); thread 0 leaves the two counts.  It
//                   carries another prefix because tests/test_nominated_cpu.py counts the k_nm_* set.
// The victim search reads the table through NomView and pre_nominees<S> (bs_preempt.hpp); with no table, or an empty one, the view is null.
// Lanes are indexed by unrolled constants only (no scratch in any instantiation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bs_preempt.hpp"

namespace bs {

constexpr uint32_t kNmWindow = 1024;

// the table's columns in one allocation; req is [L][stride]
struct NomTab {
  uint32_t* id;
  uint32_t* node;
  int32_t* prio;
  uint32_t* pres;
  int64_t* req;
  uint32_t* nhead;          // [n]
  uint32_t* nnext;          // [stride]
  uint32_t stride;
};

struct NomDev {
  NomTab src, dst;          // the live table and the twin every change is written into
  uint32_t W;               // rows of src
  uint32_t W2;              // survivors: W - n_remove
  uint32_t N;
  // the call (one H2D block)
  const uint32_t* rem;      // [n_remove] ids that leave
  uint32_t n_remove;
  const uint32_t* ipod;     // [n_insert] resident-queue index
  const uint32_t* inode;    // [n_insert]
  const int32_t* iprio;     // [n_insert]
  uint32_t n_insert, ids;   // the inserted rows get ids + k
  uint8_t* flag;            // [W] the row leaves (zeroed before the launches)
};

__global__ __launch_bounds__(256) void k_nm_mark(NomDev a) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_remove) return;
  const uint32_t key = a.rem[i];
  uint32_t lo = 0, hi = a.W;                                // the first row whose id is >= key
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.src.id[mid] < key) lo = mid + 1u;
    else hi = mid;
  }
  if (lo < a.W && a.src.id[lo] == key) a.flag[lo] = 1;
}

template <int S>
__global__ __launch_bounds__(kNmWindow) void k_nm_move(NomDev a) {
  constexpr int L = 4 + S;
  constexpr uint32_t kWaves = kNmWindow / 64;
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t base = 0;                                        // survivors in the windows before this one (every thread keeps it)
  for (uint32_t w0 = 0; w0 < a.W; w0 += kNmWindow) {
    const uint32_t e = w0 + t;
    const bool keep = e < a.W && !a.flag[e];
    const uint64_t m = __ballot(keep);
    if (lane == 0) s_cnt[wave] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t x = 0; x < kWaves; ++x) {
      const uint32_t c = s_cnt[x];
      before += x < wave ? c : 0u;
      total += c;
    }
    const uint32_t d = base + before + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (keep && d < a.dst.stride) {
      a.dst.id[d] = a.src.id[e];
      a.dst.node[d] = a.src.node[e];
      a.dst.prio[d] = a.src.prio[e];
      a.dst.pres[d] = a.src.pres[e];
#pragma unroll
      for (int l = 0; l < L; ++l) a.dst.req[(size_t)l * a.dst.stride + d] = a.src.req[(size_t)l * a.src.stride + e];
    }
    base += total;
    __syncthreads();                                        // s_cnt is rewritten by the next window
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_nm_gather(NomDev a, PodsDev pd) {
  constexpr int L = 4 + S;
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= a.n_insert) return;
  const uint32_t p = a.ipod[k], d = a.W2 + k;
  if (p >= pd.p || d >= a.dst.stride) return;               // (the host has refused such a call)
  const uint32_t smask = S > 0 ? (uint32_t)((1ull << S) - 1ull) : 0u;
  const uint32_t pres = pd.pres[p] & smask;
  a.dst.id[d] = a.ids + k;
  a.dst.node[d] = a.inode[k];
  a.dst.prio[d] = a.iprio[k];
  a.dst.pres[d] = pres;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    int64_t v = 0;
    if (l < 3) v = pd.req[(size_t)l * pd.p + p];
    else if (l == 3) v = 1;
    else if ((pres >> (l - 4)) & 1u) v = pd.req[(size_t)l * pd.p + p];
    a.dst.req[(size_t)l * a.dst.stride + d] = v;
  }
}

// bs_nominated_nodes_apply: the live table, the twin, the removed OLD nodes and where the dropped rows go
struct NomNodesDev {
  NomTab src, dst;
  uint32_t W;               // rows of src
  const uint32_t* rem;      // [R] OLD node indices that leave, ascending, distinct (one H2D block)
  uint32_t R;
  uint32_t* o_id;           // [W] the dropped rows in ascending id: id, OLD node, priority
  uint32_t* o_node;
  int32_t* o_prio;
  uint32_t* info;           // [2] survivors, dropped rows
};

template <int S>
__global__ __launch_bounds__(kNmWindow) void k_nn_move(NomNodesDev a) {
  constexpr int L = 4 + S;
  constexpr uint32_t kWaves = kNmWindow / 64;
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t base = 0;                                        // survivors in the windows before this one (every thread keeps it)
  for (uint32_t w0 = 0; w0 < a.W; w0 += kNmWindow) {
    const uint32_t e = w0 + t;
    const bool in = e < a.W;
    const uint32_t k = in ? a.src.node[e] : 0u;
    uint32_t lo = 0, hi = in ? a.R : 0u;                    // removed nodes below k
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.rem[mid] < k) lo = mid + 1u;
      else hi = mid;
    }
    const bool gone = in && lo < a.R && a.rem[lo] == k;
    const bool keep = in && !gone;
    const uint64_t m = __ballot(keep);
    if (lane == 0) s_cnt[wave] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t x = 0; x < kWaves; ++x) {
      const uint32_t c = s_cnt[x];
      before += x < wave ? c : 0u;
      total += c;
    }
    const uint32_t d = base + before + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));   // survivors in front of row e
    if (keep && d < a.dst.stride) {
      a.dst.id[d] = a.src.id[e];
      a.dst.node[d] = k - lo;
      a.dst.prio[d] = a.src.prio[e];
      a.dst.pres[d] = a.src.pres[e];
#pragma unroll
      for (int l = 0; l < L; ++l) a.dst.req[(size_t)l * a.dst.stride + d] = a.src.req[(size_t)l * a.src.stride + e];
    }
    if (gone) {                                             // (d <= e: the output row lies inside [0, W))
      const uint32_t r = e - d;
      a.o_id[r] = a.src.id[e];
      a.o_node[r] = k;
      a.o_prio[r] = a.src.prio[e];
    }
    base += total;
    __syncthreads();                                        // s_cnt is rewritten by the next window
  }
  if (t == 0) {
    a.info[0] = base;
    a.info[1] = a.W - base;
  }
}

// BS_PREEMPT_CLEAR_LOWER (include/bsched.h, rule C): the rows a plan cleared, listed behind its resolve (k_nc_resolve, bs_preempt_clear.hpp).
// thr[k] is the biased threshold word of node k (priority ^ 0x80000000, 0 = nobody stands on the node), first[k] the first standing
// slot + 1, sorig the slot's position in the caller's arrays.
struct NomClearDev {
  NomTab src;               // the live table (read only)
  uint32_t W, N;
  const uint32_t* thr;      // [n]
  const uint32_t* first;    // [n]
  const uint32_t* sorig;    // [q]
  uint32_t* o_id;           // [W] the cleared rows in ascending id: id, node, priority, the preemptor that cleared them
  uint32_t* o_node;
  int32_t* o_prio;
  uint32_t* o_by;
  uint32_t* o_count;        // [1]
};

//   k_nc_list       k_nm_move's walk (ONE workgroup, windows of 1024, a running base) with another test and nothing moved: row e is cleared
//                   iff its priority is below its node's threshold (unsigned compare of the biased words); a cleared row goes to output
//                   row base + (cleared rows in front of it inside the window); thread 0 leaves the count.  No lanes: one instantiation.
//                   (The prefix is not k_nm_: tests/test_nominated_cpu.py counts that set.)
__global__ __launch_bounds__(kNmWindow) void k_nc_list(NomClearDev a) {
  constexpr uint32_t kWaves = kNmWindow / 64;
  __shared__ uint32_t s_cnt[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint32_t base = 0;                                        // cleared rows in the windows before this one (every thread keeps it)
  for (uint32_t w0 = 0; w0 < a.W; w0 += kNmWindow) {
    const uint32_t e = w0 + t;
    const bool in = e < a.W;
    const uint32_t k = in ? a.src.node[e] : 0u;
    const int32_t p = in ? a.src.prio[e] : 0;
    const bool gone = in && k < a.N && ((uint32_t)p ^ 0x80000000u) < a.thr[k];
    const uint64_t m = __ballot(gone);
    if (lane == 0) s_cnt[wave] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t x = 0; x < kWaves; ++x) {
      const uint32_t c = s_cnt[x];
      before += x < wave ? c : 0u;
      total += c;
    }
    if (gone) {                                             // (d <= e: the output row lies inside [0, W))
      const uint32_t d = base + before + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      const uint32_t f = a.first[k];                        // (a raised threshold has a first slot)
      a.o_id[d] = a.src.id[e];
      a.o_node[d] = k;
      a.o_prio[d] = p;
      a.o_by[d] = f ? a.sorig[f - 1u] : 0xFFFFFFFFu;
    }
    base += total;
    __syncthreads();                                        // s_cnt is rewritten by the next window
  }
  if (t == 0) a.o_count[0] = base;
}

// rows of the table `t` (the new one): every row pushes itself onto its node's chain; the first thread writes the view of `t` the victim
// search reads (it lives in t's allocation)
__global__ __launch_bounds__(256) void k_nm_chains(NomTab t, NomView* view, uint32_t rows, uint32_t n) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e == 0u) *view = NomView{t.nhead, t.nnext, t.prio, t.req, t.stride};
  if (e >= rows || e >= t.stride) return;
  const uint32_t k = t.node[e];
  if (k >= n) return;                                       // (no such row: the host checks every node)
  t.nnext[e] = __hip_atomic_exchange(&t.nhead[k], e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace bs
