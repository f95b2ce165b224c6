// tu_preempt.hip — translation unit of everything over the bound-pod table.  Kernels: the preemption victim search (bs_preempt.hpp: k_preempt_scan /
// k_preempt_pick), the sequential plans (bs_preempt_commit.hpp: k_pc_*), the table's patch (bs_bound_apply.hpp: k_ba_*) and its remap after node-list
// surgery (bs_bound_nodes.hpp: k_bn_*), one instantiation per scalar-lane count 0..BS_MAX_SCALARS, and the resident PodDisruptionBudgets (bs_pdb.hpp:
// k_pdb_*, no templates), and the resident nominated-pod table (bs_nominated.hpp: k_nm_*).  Host: their file-local launch wrappers and the entry points bs_bound_*, bs_pdb_*, bs_nominated_*, bs_preempt_* (include/bsched.h).
#ifndef BS_UNITY
#define BS_TU_PREEMPT
#endif
#include "bs_preempt.hpp"
#include "bs_preempt_commit.hpp"
#include "bs_preempt_commit_gang.hpp"
#include "bs_bound_apply.hpp"
#include "bs_bound_nodes.hpp"
#include "bs_pdb.hpp"
#include "bs_nominated.hpp"
#include "bs_preempt_gang_runs.hpp"
#include "bs_preempt_geom.hpp"
#include "bs_bound_nodes_replay.hpp"
#include "bs_nominated_check.hpp"
#include "bs_ctx.hpp"

#include <cstring>
#include <iterator>
#include <type_traits>

namespace {

// the victim search: k_preempt_scan<S> over scan_grid, then k_preempt_pick<S>, one wave per preemptor
void launch_preempt(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const PreemptDev& pe) {
  lanes_wide(S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_preempt_scan<decltype(s)::value>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_preempt_pick<decltype(s)::value>), dim3(pe.q), dim3(64), 0, stream, nd, pd, pe);
  });
}

// the sequential plan: k_pc_scan<S> over scan_grid, then k_pc_resolve<S>, one workgroup
void launch_preempt_commit(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe) {
  lanes_wide(S, [&](auto s) {
    constexpr int V = decltype(s)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_scan<V>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_resolve<V>), dim3(1), dim3(pc_threads<V>()), 0, stream, nd, pd, pe);
  });
}

// bs_preempt_commit_gang's plan: k_pc_scan<S> as above, then k_gang_resolve<S> (the quorum of each gang's run, the rollback)
void launch_preempt_commit_gang(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe,
                                const GangDev& gd) {
  lanes_wide(S, [&](auto s) {
    constexpr int V = decltype(s)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_scan<V>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gang_resolve<V>), dim3(1), dim3(pc_threads<V>()), 0, stream, nd, pd, pe, gd);
  });
}

// what BS_PREEMPT_APPLY launches after a plan: k_pc_nodes<S> (ndirty records into reqs), k_pc_boff<S> + k_pc_compact<S> when nw is set
template <int S>
void launch_preempt_apply_s(hipStream_t stream, const NodesDev& nd, const CommitDev& pe, uint32_t ndirty, uint32_t assume, bs_node_request* reqs,
                                   const CompactDev* nw) {
  if (ndirty) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_nodes<S>), dim3((ndirty + 255) / 256), dim3(256), 0, stream, nd, pe, ndirty, assume, reqs);
  if (nw) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_boff<S>), dim3(1), dim3(1024), 0, stream, pe, nd.n, nw->boff);
    if (nd.n) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_compact<S>), dim3(nd.n), dim3(64), 0, stream, pe, *nw, nd.n);
  }
}
void launch_preempt_apply(hipStream_t stream, uint32_t S, const NodesDev& nd, const CommitDev& pe, uint32_t ndirty, uint32_t assume, bs_node_request* reqs,
                          const CompactDev* nw) {
  lanes_wide(S, [&](auto s) { launch_preempt_apply_s<decltype(s)::value>(stream, nd, pe, ndirty, assume, reqs, nw); });
}

// the bound table's patch (bs_bound_apply.hpp): k_ba_scatter<S>, k_ba_mark<S>, k_ba_boff<S> (the new CSR into nw.boff), k_ba_merge<S> (one wave per
// node into nw; writes nothing when the error word is set)
template <int S>
void launch_bound_apply_s(hipStream_t stream, const BoundApplyDev& a, const CompactDev& nw) {
  const uint32_t items = a.n_remove > a.n_insert ? a.n_remove : a.n_insert;
  if (a.b) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_scatter<S>), dim3((a.b + 255) / 256), dim3(256), 0, stream, a);
  if (items) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_mark<S>), dim3((items + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_boff<S>), dim3(1), dim3(1024), 0, stream, a, nw.boff);
  if (a.n) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_merge<S>), dim3((a.n + 3) / 4), dim3(256), 0, stream, a, nw);
}
void launch_bound_apply(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const CompactDev& nw) {
  lanes_wide(S, [&](auto s) { launch_bound_apply_s<decltype(s)::value>(stream, a, nw); });
}

// BS_BOUND_NODES, after the error word came back clear: k_ba_nodes<S> (one wave per node; the touched nodes' new request vectors as
// bs_node_request records for k_nodes_assume, counted in o.count)
void launch_bound_apply_nodes(hipStream_t stream, uint32_t S, const BoundApplyDev& a, const BoundNodesReqDev& o) {
  if (a.n) lanes_wide(S, [&](auto s) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ba_nodes<decltype(s)::value>), dim3((a.n + 3) / 4), dim3(256), 0, stream, a, o); });
}

// the bound table's remap after node-list surgery (bs_bound_nodes.hpp): k_bn_len<S>, k_bn_scan1<S> + k_bn_scan2<S> (the new CSR and the dropped
// ids' offsets, a.nblk blocks each), k_bn_move<S> (one wave per new node, and per removed node when ids are asked for)
template <int S>
void launch_bound_nodes_s(hipStream_t stream, const BoundNodesDev& a) {
  const uint32_t items = a.n1 > a.nrem ? a.n1 : a.nrem, waves = a.n1 + (a.dropped_cap ? a.nrem : 0u);
  if (items) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_len<S>), dim3((items + 255) / 256), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_scan1<S>), dim3(a.nblk, 2), dim3(1024), 0, stream, a);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_scan2<S>), dim3(a.nblk, 2), dim3(1024), 0, stream, a);
  if (waves) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bn_move<S>), dim3((waves + 3) / 4), dim3(256), 0, stream, a);
}
void launch_bound_nodes(hipStream_t stream, uint32_t S, const BoundNodesDev& a) {
  lanes_wide(S, [&](auto s) { launch_bound_nodes_s<decltype(s)::value>(stream, a); });
}

// resident PodDisruptionBudgets (bs_pdb.hpp): k_pdb_allowed when a.count pairs are staged, then k_pdb_bits, one wave per node of the live table,
// rewrites its PDB byte column and per-node violating counts in place
void launch_pdb(hipStream_t stream, const PdbDev& a) {
  if (a.count) hipLaunchKernelGGL(k_pdb_allowed, dim3((a.count + 255) / 256), dim3(256), 0, stream, a);
  if (a.n) hipLaunchKernelGGL(k_pdb_bits, dim3((a.n + 3) / 4), dim3(256), 0, stream, a);
}

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

// -------------------------------------------------------------------------------------------------
// the resident nominated-pod table (bs_nominated.hpp)
// -------------------------------------------------------------------------------------------------
// the table's one allocation for `cap` rows on n nodes: columns at 256-byte offsets, req lane stride max(cap, 1)
struct NomLayout {
  Piece<uint32_t> id, node;
  Piece<int32_t> prio;
  Piece<uint32_t> pres;
  Piece<int64_t> req;
  Piece<uint32_t> nhead, nnext;
  Piece<NomView> view;                 // what the victim search reads, written with the chains
  size_t bytes = 0;
  uint32_t stride = 1;
};
NomLayout nom_layout(uint32_t cap, uint32_t n, uint32_t L) {
  const size_t rows = std::max<uint32_t>(cap, 1);
  NomLayout l;
  Carve cv;
  l.id = cv.take<uint32_t>(rows);
  l.node = cv.take<uint32_t>(rows);
  l.prio = cv.take<int32_t>(rows);
  l.pres = cv.take<uint32_t>(rows);
  l.req = cv.take<int64_t>(rows * L);
  l.nhead = cv.take<uint32_t>(std::max<uint32_t>(n, 1));
  l.nnext = cv.take<uint32_t>(rows);
  l.view = cv.take<NomView>(1);
  l.bytes = cv.mark();
  l.stride = (uint32_t)rows;
  return l;
}
NomTab nom_tab(const bs_ctx* c, uint32_t which) {
  const NomLayout l = nom_layout(c->nom_cap[which], c->nom_ncap[which], c->L);
  void* b = c->d_nom[which].p;
  return NomTab{l.id.in(b), l.node.in(b), l.prio.in(b), l.pres.in(b), l.req.in(b), l.nhead.in(b), l.nnext.in(b), l.stride};
}
// allocation `which` is laid out for at least `rows` rows on the context's nodes afterwards (a quarter of headroom, as the wait table);
// what it held is lost when the layout changes
hipError_t nom_reserve(bs_ctx* c, uint32_t which, uint32_t rows) {
  if (c->d_nom[which].p && c->nom_cap[which] >= rows && c->nom_ncap[which] == c->N) return hipSuccess;
  const uint32_t cap = std::max<uint32_t>(rows + rows / 4, 256);
  const hipError_t e = c->d_nom[which].reserve(nom_layout(cap, c->N, c->L).bytes);
  if (e == hipSuccess) { c->nom_cap[which] = cap; c->nom_ncap[which] = c->N; }
  return e;
}
// what the victim search reads: null without a table or without rows (the callers have refused a stale table that holds rows)
const NomView* nom_view(const bs_ctx* c) {
  if (!c->have_nom || c->nom_w == 0) return nullptr;
  const uint32_t cur = c->nom_cur;
  return nom_layout(c->nom_cap[cur], c->nom_ncap[cur], c->L).view.in((const void*)c->d_nom[cur].p);
}
// the chains of allocation `which` over `rows` rows: nhead filled with kNmNone, then k_nm_chains, which also writes the view of that table
// (a table without rows has no view: nom_view answers null for it)
hipError_t launch_nom_chains(bs_ctx* c, uint32_t which, uint32_t rows) {
  const NomTab t = nom_tab(c, which);
  NomView* dv = nom_layout(c->nom_cap[which], c->nom_ncap[which], c->L).view.in(c->d_nom[which].p);
  const hipError_t e = hipMemsetAsync(t.nhead, 0xff, (size_t)std::max<uint32_t>(c->N, 1) * 4, c->stream);
  if (e == hipSuccess && rows) hipLaunchKernelGGL(k_nm_chains, dim3(cdiv(rows, 256)), dim3(256), 0, c->stream, t, dv, rows, c->N);
  return e;
}
// k_nm_mark -> k_nm_move<S> (one workgroup) -> k_nm_gather<S>; the chains follow (launch_nom_chains)
void launch_nom_apply(hipStream_t stream, uint32_t S, const NomDev& a, const PodsDev& pd) {
  if (a.n_remove) hipLaunchKernelGGL(k_nm_mark, dim3(cdiv(a.n_remove, 256)), dim3(256), 0, stream, a);
  lanes_wide(S, [&](auto s) {
    constexpr int V = decltype(s)::value;
    if (a.W) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_move<V>), dim3(1), dim3(kNmWindow), 0, stream, a);
    if (a.n_insert) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_gather<V>), dim3(cdiv(a.n_insert, 256)), dim3(256), 0, stream, a, pd);
  });
}
int nom_single_rank(bs_ctx* c, const char* who) {
  if (c->nranks > 1 || c->reduce_external) { c->last_error = std::string(who) + " is single-rank only (as bs_preempt_run)"; return BS_ERR_STATE; }
  return BS_OK;
}
// the table exists and was made for the node count the context holds now
int nom_state(bs_ctx* c, const char* who) {
  if (const int rc = nom_single_rank(c, who)) return rc;
  if (!c->have_nom) { c->last_error = std::string(who) + ": no nominated-pod table (bs_nominated_load first; m = 0 gives the empty one)"; return BS_ERR_STATE; }
  if (!c->have_nodes || c->nom_n != c->N) {
    c->last_error = std::string(who) + ": the nominated-pod table was made for another node count (bs_nominated_read before the surgery, a remap on the host, bs_nominated_load)";
    return BS_ERR_STATE;
  }
  return BS_OK;
}
// what the three preemption calls refuse: rows of a table that was made for another node count
int nom_preempt_state(bs_ctx* c, const char* who) {
  if (c->have_nom && c->nom_w && c->nom_n != c->N) {
    c->last_error = std::string(who) + ": the nominated-pod table holds rows and was made for another node count: reload it";
    return BS_ERR_STATE;
  }
  return BS_OK;
}
int nom_refusal(bs_ctx* c, const char* who, int bad) {
  c->last_error = std::string(who) + ": " + nom_check_text(bad);
  return nom_check_is_capacity(bad) ? BS_ERR_CAPACITY : BS_ERR_INVALID;
}
// bs_nominated_apply behind its checks (and BS_PREEMPT_NOMINATE's append): the listed rows leave by the stable compaction into the twin,
// the inserts are gathered from the resident queue behind the survivors, the chains are rebuilt, the twin becomes the table.  One wait.
int nom_apply_rows(bs_ctx* c, uint32_t R, const uint32_t* remove_id, uint32_t I, const uint32_t* pod_index, const uint32_t* node,
                   const int32_t* priority) {
  const uint32_t W = c->nom_w, W2 = W - R, W3 = W2 + I, cur = c->nom_cur, other = cur ^ 1u, ids = c->nom_ids;
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (nothing of an earlier call still reads the twin)
  HIPCHK(c, nom_reserve(c, other, W3));
  const size_t nR = R, nI = I;
  Carve cv;
  const auto o_rem = cv.take<uint32_t>(nR, 4);              // (packed: one H2D)
  const auto o_pod = cv.take<uint32_t>(nI, 4);
  const auto o_node = cv.take<uint32_t>(nI, 4);
  const auto o_prio = cv.take<int32_t>(nI, 4);
  const size_t blob_bytes = cv.mark();
  const auto o_flag = cv.take<uint8_t>(std::max<uint32_t>(W, 1));
  if (cv.mark() > c->d_pre.cap) HIPCHK(c, c->d_pre.reserve(cv.mark() + cv.mark() / 4));
  std::vector<uint8_t> h(std::max<size_t>(blob_bytes, 1), 0);
  if (R) std::memcpy(o_rem.in(h.data()), remove_id, o_rem.bytes());
  if (I) {
    std::memcpy(o_pod.in(h.data()), pod_index, o_pod.bytes());
    std::memcpy(o_node.in(h.data()), node, o_node.bytes());
    std::memcpy(o_prio.in(h.data()), priority, o_prio.bytes());
  }
  uint8_t* base = c->d_pre.as<uint8_t>();
  HIPCHK(c, hipMemcpyAsync(base, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(o_flag.in(base), 0, o_flag.bytes(), c->stream));
  NomDev a{};
  a.src = nom_tab(c, cur);
  a.dst = nom_tab(c, other);
  a.W = W; a.W2 = W2; a.N = c->N;
  a.rem = o_rem.in(base);
  a.n_remove = R;
  a.ipod = o_pod.in(base);
  a.inode = o_node.in(base);
  a.iprio = o_prio.in(base);
  a.n_insert = I;
  a.ids = ids;
  a.flag = o_flag.in(base);
  launch_nom_apply(c->stream, c->S, a, pods_dev(c));
  HIPCHK(c, launch_nom_chains(c, other, W3));
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (h is a local buffer)
  if (R) {
    std::vector<uint32_t> gone(remove_id, remove_id + R), left;
    std::sort(gone.begin(), gone.end());
    left.reserve(W3);
    std::set_difference(c->nom_live.begin(), c->nom_live.end(), gone.begin(), gone.end(), std::back_inserter(left));
    c->nom_live.swap(left);
  }
  for (uint32_t k = 0; k < I; ++k) c->nom_live.push_back(ids + k);
  c->nom_cur = other;
  c->nom_w = W3;
  c->nom_ids = ids + I;
  return BS_OK;
}

}  // namespace

int32_t* bs::bound_group_column(const bs_ctx* c) { return bound_cols(c->d_bound.as<uint8_t>(), c->blay).group; }

// the back half of every patch of the bound table (bs_ctx.hpp): the second allocation, the merge chain over a delta block that is on the
// device, the one wait, the error word, the swap
int bs::bound_apply_block(bs_ctx* c, const char* who, BoundApplyDev& a, int32_t gmax, const BoundBlockHooks* hooks) {
  const uint32_t N = c->N, L = c->L, B = c->bound_b, ids = c->bound_ids, R = a.n_remove, I = a.n_insert;
  const uint32_t B2 = B - R + I;                           // (when the error word stays clear)
  BoundLayout lay{};
  const size_t table_bytes = bound_layout(L, N, B2, lay);
  if (table_bytes > c->d_bound2.cap) HIPCHK(c, c->d_bound2.reserve(table_bytes + table_bytes / 4));
  const auto bt = bound_dev(a, c->d_bound.as<const uint8_t>(), c->blay);
  a.bpres = bt.pres;
  a.bstride = std::max<uint32_t>(B, 1);
  a.b = B; a.n = N; a.ids = ids;
  CompactDev nw{};
  const auto nt = bound_dev(nw, c->d_bound2.as<uint8_t>(), lay);
  nw.bpres = nt.pres;
  nw.bnviol = nt.nviol;
  nw.bstride = std::max<uint32_t>(B2, 1);
  launch_bound_apply(c->stream, c->S, a, nw);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  if (hooks && hooks->before_wait)
    if (const int rc = hooks->before_wait()) return rc;
  uint32_t err = 0;                                        // read before the swap: the merge wrote nothing when it is set
  HIPCHK(c, hipMemcpyAsync(&err, a.err, sizeof err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hooks && hooks->verdict)
    if (const int rc = hooks->verdict(err, gmax)) return rc;
  if (err & (kBaErrUnknown | kBaErrDead | kBaErrTwice | kBaErrNode)) {
    c->last_error = std::string(who) + ((err & kBaErrTwice) ? ": a remove id is listed twice"
                                        : (err & kBaErrDead) ? ": a remove id is not live (evicted or removed earlier)"
                                                             : ": a remove id or an insert node is out of range");
    return BS_ERR_INVALID;
  }
  if (err & kBaErrFull) { c->last_error = std::string(who) + ": more than BS_BOUND_MAX_PER_NODE bound pods on one node"; return BS_ERR_CAPACITY; }
  std::swap(c->d_bound.p, c->d_bound2.p);
  std::swap(c->d_bound.cap, c->d_bound2.cap);
  c->blay = lay;
  c->bound_b = B2;
  c->bound_ids = ids + I;
  c->bound_max_group = gmax;
  return BS_OK;
}

extern "C" {
int bs_bound_load(bs_ctx* c, const bs_bound_soa* bd) {
  if (!c || !bd) return BS_ERR_INVALID;
  if (!c->have_nodes) { c->last_error = "bs_bound_load before bs_nodes_load"; return BS_ERR_STATE; }
  const uint32_t B = bd->b, N = c->N, L = c->L;
  if (B > BS_BOUND_MAX) { c->last_error = "bound table larger than BS_BOUND_MAX"; return BS_ERR_CAPACITY; }
  if (B && (!bd->node || !bd->priority || !bd->start_ns || !bd->group || !bd->req || !bd->req_present)) return BS_ERR_INVALID;
  std::vector<uint32_t> cnt((size_t)N + 1, 0);
  int32_t gmax = -1;
  for (uint32_t i = 0; i < B; ++i) {
    if (bd->node[i] >= N) { c->last_error = "bound pod on a node index >= n"; return BS_ERR_INVALID; }
    if (bd->group[i] < BS_POD_GROUP_MISSING) { c->last_error = "bound pod group index below BS_POD_GROUP_MISSING"; return BS_ERR_INVALID; }
    gmax = std::max(gmax, bd->group[i]);
    ++cnt[bd->node[i] + 1];
  }
  for (uint32_t k = 0; k < N; ++k) {
    if (cnt[k + 1] > BS_BOUND_MAX_PER_NODE) { c->last_error = "more than BS_BOUND_MAX_PER_NODE bound pods on one node"; return BS_ERR_CAPACITY; }
    cnt[k + 1] += cnt[k];
  }
  int rc = use_device(c);
  if (rc) return rc;
  // every node's pods in importance order: priority descending, start ascending, caller id ascending
  std::vector<uint32_t> order(B), fill(cnt.begin(), cnt.end() - 1);
  for (uint32_t i = 0; i < B; ++i) order[fill[bd->node[i]]++] = i;
  for (uint32_t k = 0; k < N; ++k)
    std::sort(order.begin() + cnt[k], order.begin() + cnt[k + 1], [&](uint32_t a, uint32_t b) {
      if (bd->priority[a] != bd->priority[b]) return bd->priority[a] > bd->priority[b];
      if (bd->start_ns[a] != bd->start_ns[b]) return bd->start_ns[a] < bd->start_ns[b];
      return a < b;
    });
  const size_t nB = std::max<uint32_t>(B, 1);
  BoundLayout lay;
  const size_t o = bound_layout(L, N, B, lay);
  c->blay = lay;
  std::vector<uint8_t> h(o, 0);
  const auto ht = bound_cols(h.data(), lay);
  std::memcpy(ht.boff, cnt.data(), ((size_t)N + 1) * 4);
  const uint32_t smask = (uint32_t)((1ull << (L - BS_FIXED_LANES)) - 1ull);
  for (uint32_t r = 0; r < B; ++r) {
    const uint32_t i = order[r];
    ht.pres[r] = bd->req_present[i] & smask;
    ht.prio[r] = bd->priority[i];
    ht.start[r] = bd->start_ns[i];
    ht.group[r] = bd->group[i];
    ht.id[r] = i;
    for (uint32_t l = 0; l < L; ++l) {
      int64_t v = bd->req[(size_t)l * B + i];
      if (l == BS_LANE_PODS) v = 1;                                        // RemovePod: one pod less
      else if (l >= BS_FIXED_LANES && !((bd->req_present[i] >> (l - BS_FIXED_LANES)) & 1u)) v = 0;   // no key: nothing to subtract
      ht.req[(size_t)l * nB + r] = v;
    }
  }
  c->have_bound = false;
  HIPCHK(c, c->d_bound.reserve(o));
  HIPCHK(c, hipMemcpyAsync(c->d_bound.p, h.data(), o, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));             // (h is a local buffer)
  c->bound_b = B;
  c->bound_ids = B;
  c->bound_n = N;
  c->bound_max_group = gmax;
  c->have_bound = true;                                   // (h was zeroed: every PDB bit is clear)
  c->have_pdb = false;                                    // the id space restarts: the resident PDB state names the old one
  c->pdb_n = c->pdb_covered = c->pdb_members = 0;
  return BS_OK;
}

int bs_bound_pdb_set(bs_ctx* c, uint32_t b, const uint8_t* violating) {
  if (!c) return BS_ERR_INVALID;
  if (!c->have_bound) { c->last_error = "bs_bound_pdb_set before bs_bound_load"; return BS_ERR_STATE; }
  if (b != c->bound_ids) { c->last_error = "bs_bound_pdb_set: b differs from the last bs_bound_load's entry count"; return BS_ERR_INVALID; }
  const uint32_t B = c->bound_b, N = c->bound_n;
  int rc = use_device(c);
  if (rc) return rc;
  const auto bt = bound_cols(c->d_bound.as<uint8_t>(), c->blay);
  const size_t nB = std::max<uint32_t>(B, 1), nN = std::max<uint32_t>(N, 1);
  // the two columns are rebuilt on the host through the id column (the id -> position map; evicted ids are not in it) and copied in
  // stream order, behind whatever preemption call is still running
  std::vector<uint8_t> bits(nB, 0);
  std::vector<uint32_t> nviol(nN, 0);
  if (violating && B) {
    std::vector<uint32_t> boff((size_t)N + 1), id(B);
    HIPCHK(c, hipMemcpyAsync(boff.data(), bt.boff, ((size_t)N + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(id.data(), bt.id, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < N; ++k)
      for (uint32_t j = boff[k]; j < boff[k + 1] && j < B; ++j) {
        bits[j] = id[j] < b && violating[id[j]] ? 1 : 0;
        nviol[k] += bits[j];
      }
  }
  HIPCHK(c, hipMemcpyAsync(bt.pdb, bits.data(), nB, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(bt.nviol, nviol.data(), nN * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));             // (local buffers)
  return BS_OK;
}

// -------------------------------------------------------------------------------------------------
// resident PodDisruptionBudgets (bs_pdb.hpp): the PDB bits follow the budgets' status on the device
// -------------------------------------------------------------------------------------------------
namespace {

// what every bs_pdb_* call refuses before it looks at its arguments
int pdb_state(bs_ctx* c, const char* who, bool need_pdb) {
  if (!c->have_bound) { c->last_error = std::string(who) + " before bs_bound_load"; return BS_ERR_STATE; }
  if (c->nranks > 1 || c->reduce_external) { c->last_error = std::string(who) + " is single-rank only"; return BS_ERR_STATE; }
  if (need_pdb && !c->have_pdb) { c->last_error = std::string(who) + " without a bs_pdb_load since the last bs_bound_load"; return BS_ERR_STATE; }
  return BS_OK;
}

// member_off[n + 1] ascending from 0, every member < n_pdb, and the total within BS_PDB_MEMBERS_MAX on top of `have`
int pdb_csr_check(bs_ctx* c, const char* who, uint32_t n, const uint32_t* member_off, const uint32_t* member, uint32_t n_pdb, uint32_t have) {
  if (n && !member_off) return BS_ERR_INVALID;
  const uint32_t total = n ? member_off[n] : 0u;
  if (n && member_off[0] != 0u) { c->last_error = std::string(who) + ": member_off does not start at 0"; return BS_ERR_INVALID; }
  for (uint32_t i = 0; i < n; ++i)
    if (member_off[i + 1] < member_off[i]) { c->last_error = std::string(who) + ": member_off is not ascending"; return BS_ERR_INVALID; }
  if ((uint64_t)have + total > BS_PDB_MEMBERS_MAX) { c->last_error = std::string(who) + ": more than BS_PDB_MEMBERS_MAX membership entries"; return BS_ERR_CAPACITY; }
  if (total && !member) return BS_ERR_INVALID;
  for (uint32_t x = 0; x < total; ++x)
    if (member[x] >= n_pdb) { c->last_error = std::string(who) + ": a member index >= n_pdb"; return BS_ERR_INVALID; }
  return BS_OK;
}

// the recompute behind whatever the caller enqueued (count staged pairs go into allowed[] first); waits for it
int pdb_recompute(bs_ctx* c, uint32_t count, const uint32_t* index, const int32_t* value) {
  PdbDev a{};
  const auto bt = bound_cols(c->d_bound.as<uint8_t>(), c->blay);
  a.boff = bt.boff; a.bid = bt.id; a.bpdb = bt.pdb; a.bnviol = bt.nviol;
  a.n = c->bound_n;
  a.moff = c->d_pdb_moff.as<uint32_t>();
  a.member = c->d_pdb_member.as<uint32_t>();
  a.allowed = c->d_pdb_allowed.as<int32_t>();
  a.covered = c->pdb_covered;
  a.index = index;
  a.value = value;
  a.count = count;
  launch_pdb(c->stream, a);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BS_OK;
}

// room for `bytes` in a buffer whose first `keep` bytes stay: a buffer that has to grow gets a quarter of headroom (a run of appends
// allocates rarely, as the bound table does)
int pdb_grow(bs_ctx* c, DevBuf& buf, size_t bytes, size_t keep) {
  if (bytes <= buf.cap) return BS_OK;
  DevBuf nw;
  HIPCHK(c, nw.reserve(bytes + bytes / 4));
  if (keep) HIPCHK(c, hipMemcpyAsync(nw.p, buf.p, keep, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::swap(buf.p, nw.p);
  std::swap(buf.cap, nw.cap);
  return BS_OK;                                            // (nw frees the old allocation)
}

}  // namespace

int bs_pdb_load(bs_ctx* c, uint32_t n_pdb, const int32_t* allowed, uint32_t b, const uint32_t* member_off, const uint32_t* member) {
  if (!c) return BS_ERR_INVALID;
  int rc = pdb_state(c, "bs_pdb_load", false);
  if (rc) return rc;
  if (n_pdb > BS_PDB_MAX) { c->last_error = "bs_pdb_load: more than BS_PDB_MAX PDBs"; return BS_ERR_CAPACITY; }
  if (b != c->bound_ids) { c->last_error = "bs_pdb_load: b differs from bs_bound_ids"; return BS_ERR_INVALID; }
  if (n_pdb && !allowed) return BS_ERR_INVALID;
  if ((rc = pdb_csr_check(c, "bs_pdb_load", b, member_off, member, n_pdb, 0u))) return rc;
  if ((rc = use_device(c))) return rc;
  const uint32_t total = b ? member_off[b] : 0u, zero = 0;
  c->have_pdb = false;
  HIPCHK(c, c->d_pdb_allowed.reserve((size_t)std::max<uint32_t>(n_pdb, 1) * 4));
  HIPCHK(c, c->d_pdb_moff.reserve(((size_t)b + 1) * 4));
  HIPCHK(c, c->d_pdb_member.reserve((size_t)std::max<uint32_t>(total, 1) * 4));
  if (n_pdb) HIPCHK(c, hipMemcpyAsync(c->d_pdb_allowed.p, allowed, (size_t)n_pdb * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_pdb_moff.p, b ? member_off : &zero, ((size_t)b + 1) * 4, hipMemcpyHostToDevice, c->stream));
  if (total) HIPCHK(c, hipMemcpyAsync(c->d_pdb_member.p, member, (size_t)total * 4, hipMemcpyHostToDevice, c->stream));
  c->pdb_n = n_pdb;
  c->pdb_covered = b;
  c->pdb_members = total;
  if ((rc = pdb_recompute(c, 0u, nullptr, nullptr))) return rc;   // (waits: the caller's arrays and `zero` are free again)
  c->have_pdb = true;
  return BS_OK;
}

int bs_pdb_members_append(bs_ctx* c, uint32_t first_id, uint32_t n, const uint32_t* member_off, const uint32_t* member) {
  if (!c) return BS_ERR_INVALID;
  int rc = pdb_state(c, "bs_pdb_members_append", true);
  if (rc) return rc;
  if (first_id != c->pdb_covered) { c->last_error = "bs_pdb_members_append: first_id differs from the number of ids covered so far"; return BS_ERR_INVALID; }
  if ((uint64_t)first_id + n > c->bound_ids) { c->last_error = "bs_pdb_members_append: first_id + n passes bs_bound_ids"; return BS_ERR_INVALID; }
  if ((rc = pdb_csr_check(c, "bs_pdb_members_append", n, member_off, member, c->pdb_n, c->pdb_members))) return rc;
  if ((rc = use_device(c))) return rc;
  const uint32_t total = n ? member_off[n] : 0u, have = c->pdb_members, cov = c->pdb_covered;
  if (n) {
    if ((rc = pdb_grow(c, c->d_pdb_moff, ((size_t)cov + n + 1) * 4, ((size_t)cov + 1) * 4))) return rc;
    if ((rc = pdb_grow(c, c->d_pdb_member, ((size_t)have + total) * 4, (size_t)have * 4))) return rc;
    std::vector<uint32_t> off(n);                          // the run's ends, moved behind the entries the CSR holds
    for (uint32_t i = 0; i < n; ++i) off[i] = have + member_off[i + 1];
    HIPCHK(c, hipMemcpyAsync(c->d_pdb_moff.as<uint32_t>() + cov + 1, off.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (total) HIPCHK(c, hipMemcpyAsync(c->d_pdb_member.as<uint32_t>() + have, member, (size_t)total * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));            // (off is a local buffer)
    c->pdb_covered = cov + n;
    c->pdb_members = have + total;
  }
  return pdb_recompute(c, 0u, nullptr, nullptr);
}

int bs_pdb_allowed_apply(bs_ctx* c, uint32_t count, const uint32_t* index, const int32_t* value) {
  if (!c) return BS_ERR_INVALID;
  int rc = pdb_state(c, "bs_pdb_allowed_apply", true);
  if (rc) return rc;
  if (count == 0) return BS_OK;
  if (!index || !value) return BS_ERR_INVALID;
  if (count > c->pdb_n) { c->last_error = "bs_pdb_allowed_apply: more pairs than PDBs (an index is listed twice or is out of range)"; return BS_ERR_INVALID; }
  std::vector<uint32_t> seen(index, index + count);
  std::sort(seen.begin(), seen.end());
  if (seen.back() >= c->pdb_n) { c->last_error = "bs_pdb_allowed_apply: an index >= n_pdb"; return BS_ERR_INVALID; }
  if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { c->last_error = "bs_pdb_allowed_apply: an index is listed twice"; return BS_ERR_INVALID; }
  if ((rc = use_device(c))) return rc;
  const size_t bytes = (size_t)count * 8;
  HIPCHK(c, c->h_pdbstage.reserve(bytes, std::max<size_t>(bytes + bytes / 4, 4096)));
  std::memcpy(c->h_pdbstage.p, index, (size_t)count * 4);
  std::memcpy(c->h_pdbstage.p + (size_t)count * 4, value, (size_t)count * 4);
  HIPCHK(c, c->h_pdbstage.mark_busy(c->stream));
  rc = pdb_recompute(c, count, reinterpret_cast<const uint32_t*>(c->h_pdbstage.p), reinterpret_cast<const int32_t*>(c->h_pdbstage.p + (size_t)count * 4));
  if (rc == BS_OK) c->h_pdbstage.busy = false;             // (the recompute waited for the stream)
  return rc;
}

int bs_pdb_read(bs_ctx* c, uint32_t* n_pdb_out, uint32_t* covered_out, int32_t* allowed_out, uint32_t* node_violating_out) {
  if (!c) return BS_ERR_INVALID;
  int rc = pdb_state(c, "bs_pdb_read", true);
  if (rc) return rc;
  if (node_violating_out && c->bound_n != c->N) { c->last_error = "the bound table was loaded for another node list: reload it"; return BS_ERR_STATE; }
  if ((rc = use_device(c))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_pdb_out) *n_pdb_out = c->pdb_n;
  if (covered_out) *covered_out = c->pdb_covered;
  if (allowed_out && c->pdb_n) HIPCHK(c, hipMemcpy(allowed_out, c->d_pdb_allowed.p, (size_t)c->pdb_n * 4, hipMemcpyDeviceToHost));
  if (node_violating_out && c->bound_n)
    HIPCHK(c, hipMemcpy(node_violating_out, bound_cols(c->d_bound.as<const uint8_t>(), c->blay).nviol, (size_t)c->bound_n * 4, hipMemcpyDeviceToHost));
  return BS_OK;
}

int bs_preempt_pdb_read(bs_ctx* c, uint32_t count, uint32_t* n_pdb_violations) {
  if (!c) return BS_ERR_INVALID;
  if (!c->have_pre_npv) { c->last_error = "bs_preempt_pdb_read before a successful bs_preempt_run / bs_preempt_commit"; return BS_ERR_STATE; }
  if (count != c->pre_npv.size()) { c->last_error = "bs_preempt_pdb_read: count differs from the last preemption call's"; return BS_ERR_INVALID; }
  if (count == 0) return BS_OK;
  if (!n_pdb_violations) return BS_ERR_INVALID;
  std::memcpy(n_pdb_violations, c->pre_npv.data(), (size_t)count * 4);
  return BS_OK;
}

int bs_preempt_nominated_read(bs_ctx* c, uint32_t count, uint32_t* id_out) {
  if (!c) return BS_ERR_INVALID;
  if (!c->have_pre_nom) { c->last_error = "bs_preempt_nominated_read: the last successful preemption call did not carry BS_PREEMPT_NOMINATE"; return BS_ERR_STATE; }
  if (count != c->pre_nom.size()) { c->last_error = "bs_preempt_nominated_read: count differs from the last preemption call's"; return BS_ERR_INVALID; }
  if (count == 0) return BS_OK;
  if (!id_out) return BS_ERR_INVALID;
  std::memcpy(id_out, c->pre_nom.data(), (size_t)count * 4);
  return BS_OK;
}

// -------------------------------------------------------------------------------------------------
// the resident nominated-pod table (bs_nominated.hpp): pods nominated by earlier cycles, counted by every fit test of the victim search
// -------------------------------------------------------------------------------------------------
int bs_nominated_load(bs_ctx* c, uint32_t m, const uint32_t* node, const int32_t* priority, const int64_t* req, const uint32_t* req_present) {
  if (!c) return BS_ERR_INVALID;
  int rc = nom_single_rank(c, "bs_nominated_load");
  if (rc) return rc;
  if (!c->have_nodes) { c->last_error = "bs_nominated_load before bs_nodes_load"; return BS_ERR_STATE; }
  if (const int bad = nom_load_check(c->N, m, node, priority, req, req_present, BS_NOM_MAX)) return nom_refusal(c, "bs_nominated_load", bad);
  if ((rc = use_device(c))) return rc;
  const uint32_t L = c->L, other = c->nom_cur ^ 1u;
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (nothing of an earlier call still reads the twin)
  HIPCHK(c, nom_reserve(c, other, m));
  const NomLayout l = nom_layout(c->nom_cap[other], c->nom_ncap[other], L);
  if (m) {
    // the columns as the table stores them: ids 0 .. m - 1, the pods lane 1, a scalar lane without a present bit 0
    std::vector<uint8_t> st(l.nhead.off);                   // (the chains are made on the device)
    const uint32_t smask = c->S ? (uint32_t)((1ull << c->S) - 1ull) : 0u;
    for (uint32_t i = 0; i < m; ++i) {
      l.id.in(st.data())[i] = i;
      l.node.in(st.data())[i] = node[i];
      l.prio.in(st.data())[i] = priority[i];
      l.pres.in(st.data())[i] = req_present[i] & smask;
    }
    for (uint32_t j = 0; j < L; ++j)
      for (uint32_t i = 0; i < m; ++i) {
        int64_t v = req[(size_t)j * m + i];
        if (j == BS_LANE_PODS) v = 1;
        else if (j >= BS_FIXED_LANES && !((req_present[i] & smask) >> (j - BS_FIXED_LANES) & 1u)) v = 0;
        l.req.in(st.data())[(size_t)j * l.stride + i] = v;
      }
    HIPCHK(c, hipMemcpyAsync(c->d_nom[other].p, st.data(), st.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_nom_chains(c, other, m));
    LAUNCHCHK(c, BS_KERNEL_PREPASS);
    HIPCHK(c, hipStreamSynchronize(c->stream));             // (st is a local buffer)
  }
  c->nom_cur = other;
  c->have_nom = true;
  c->nom_w = c->nom_ids = m;
  c->nom_n = c->N;
  c->nom_live.resize(m);
  for (uint32_t i = 0; i < m; ++i) c->nom_live[i] = i;
  return BS_OK;
}

int bs_nominated_count(const bs_ctx* c, uint32_t* m_out) {
  if (!c || !m_out) return BS_ERR_INVALID;
  if (!c->have_nom) return BS_ERR_STATE;
  *m_out = c->nom_w;
  return BS_OK;
}

int bs_nominated_ids(const bs_ctx* c, uint32_t* ids_out) {
  if (!c || !ids_out) return BS_ERR_INVALID;
  if (!c->have_nom) return BS_ERR_STATE;
  *ids_out = c->nom_ids;
  return BS_OK;
}

int bs_nominated_read(bs_ctx* c, uint32_t* id, uint32_t* node, int32_t* priority, int64_t* req, uint32_t* req_present) {
  if (!c) return BS_ERR_INVALID;
  int rc = nom_state(c, "bs_nominated_read");
  if (rc) return rc;
  const uint32_t W = c->nom_w;
  if (W && (!id || !node || !priority || !req || !req_present)) { c->last_error = "bs_nominated_read: a column is NULL and the table has rows"; return BS_ERR_INVALID; }
  if ((rc = use_device(c))) return rc;
  if (!W) return BS_OK;
  const NomTab t = nom_tab(c, c->nom_cur);
  HIPCHK(c, hipMemcpyAsync(id, t.id, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(node, t.node, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(priority, t.prio, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(req_present, t.pres, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  for (uint32_t j = 0; j < c->L; ++j)
    HIPCHK(c, hipMemcpyAsync(req + (size_t)j * W, t.req + (size_t)j * t.stride, (size_t)W * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BS_OK;
}

int bs_nominated_apply(bs_ctx* c, uint32_t n_remove, const uint32_t* remove_id, uint32_t n_insert, const uint32_t* pod_index, const uint32_t* node,
                       const int32_t* priority, uint32_t* first_id_out) {
  if (!c) return BS_ERR_INVALID;
  int rc = nom_state(c, "bs_nominated_apply");
  if (rc) return rc;
  if (n_insert && !c->have_pods) { c->last_error = "bs_nominated_apply: inserts need the pods loaded (the rows are gathered from the resident queue)"; return BS_ERR_STATE; }
  if (const int bad = nom_apply_check(c->nom_live.data(), c->nom_w, c->nom_ids, n_remove, remove_id, n_insert, pod_index, node, priority, c->P, c->N,
                                      BS_NOM_MAX, kNomMaxIds))
    return nom_refusal(c, "bs_nominated_apply", bad);
  const uint32_t ids = c->nom_ids;
  if (n_remove || n_insert) {
    if ((rc = use_device(c))) return rc;
    if ((rc = nom_apply_rows(c, n_remove, remove_id, n_insert, pod_index, node, priority))) return rc;
  }
  if (first_id_out) *first_id_out = ids;
  return BS_OK;
}

int bs_bound_count(const bs_ctx* c, uint32_t* b_out) {
  if (!c || !b_out) return BS_ERR_INVALID;
  *b_out = c->have_bound ? c->bound_b : 0u;
  return BS_OK;
}

int bs_preempt_run(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority, const uint8_t* group_protected,
                   uint32_t victim_cap, const bs_preempt_out* out) {
  if (!c || !out) return BS_ERR_INVALID;
  if (stages & ~BS_STAGE_PREFILTER) { c->last_error = "bs_preempt_run takes BS_STAGE_PREFILTER only (the plugin's Filter takes no part)"; return BS_ERR_INVALID; }
  if (!c->have_nodes || !c->have_fit || !c->have_pods || !c->have_bound) {
    c->last_error = "bs_preempt_run needs nodes, fit, pods and the bound table loaded";
    return BS_ERR_STATE;
  }
  if (c->nranks > 1 || c->reduce_external) { c->last_error = "bs_preempt_run is single-rank only"; return BS_ERR_STATE; }
  if (c->bound_n != c->N) { c->last_error = "the bound table was loaded for another node list: reload it"; return BS_ERR_STATE; }
  if (const int nrc = nom_preempt_state(c, "bs_preempt_run")) return nrc;
  if (count > BS_PREEMPT_MAX || (uint64_t)count * victim_cap > (1ull << 28)) return BS_ERR_CAPACITY;
  if (count == 0) { c->pre_npv.clear(); c->have_pre_npv = true; c->have_gang = false; c->have_pre_nom = false; return BS_OK; }
  if (!pod_index || !priority || !out->node || !out->n_victims || (victim_cap && !out->victims) || (c->G && !group_protected)) return BS_ERR_INVALID;
  if (c->bound_max_group >= (int32_t)c->G) { c->last_error = "the bound table names a group index >= the loaded group count"; return BS_ERR_INVALID; }
  const uint32_t P = c->P, N = c->N, G = c->G;
  for (uint32_t i = 0; i < count; ++i)
    if (pod_index[i] >= P) { c->last_error = "preemptor pod index >= p"; return BS_ERR_INVALID; }
  int rc = use_device(c);
  if (rc) return rc;
  // slots in priority-descending order (stable): the tile's highest priority bounds its lanes' victim suffixes
  std::vector<uint32_t> perm(count);
  for (uint32_t i = 0; i < count; ++i) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return priority[a] > priority[b]; });
  const PreemptGeom geom = preempt_geom(N, count, c->test_pc_chunk_nodes);   // slot tiles x node chunks (bs_preempt_geom.hpp)
  const uint32_t tiles = geom.tiles, nchunks = geom.nchunks, chunk_nodes = geom.chunk_nodes;
  const size_t nQ = count, nG = std::max<uint32_t>(G, 1), nR = (size_t)nchunks * nQ, nV = std::max<size_t>((size_t)nQ * victim_cap, 1);
  Carve cv;
  const auto o_spod = cv.take<uint32_t>(nQ);
  const auto o_sprio = cv.take<int32_t>(nQ);
  const auto o_sorig = cv.take<uint32_t>(nQ);
  const auto o_gprot = cv.take<uint8_t>(nG);
  const size_t in_bytes = cv.mark();
  const auto o_rnode = cv.take<int32_t>(nR);
  const auto o_rnv = cv.take<uint32_t>(nR);
  const auto o_rnpv = cv.take<uint32_t>(nR);
  const auto o_rtop = cv.take<int32_t>(nR);
  const auto o_rsum = cv.take<int64_t>(nR);
  const auto o_rest = cv.take<int64_t>(nR);
  const auto o_rncand = cv.take<uint32_t>(nR);
  const size_t o_res = cv.mark();                           // results: one D2H
  const auto o_node = cv.take<int32_t>(nQ);
  const auto o_ncand = cv.take<uint32_t>(nQ);
  const auto o_nv = cv.take<uint32_t>(nQ);
  const auto o_npv = cv.take<uint32_t>(nQ);
  const auto o_top = cv.take<int32_t>(nQ);
  const auto o_sum = cv.take<int64_t>(nQ);
  const auto o_est = cv.take<int64_t>(nQ);
  const auto o_vic = cv.take<uint32_t>(nV);
  HIPCHK(c, c->d_pre.reserve(cv.mark()));
  std::vector<uint8_t> in(in_bytes, 0);
  for (uint32_t s = 0; s < count; ++s) {
    o_spod.in(in.data())[s] = pod_index[perm[s]];
    o_sprio.in(in.data())[s] = priority[perm[s]];
    o_sorig.in(in.data())[s] = perm[s];
  }
  if (G) std::memcpy(o_gprot.in(in.data()), group_protected, G);
  uint8_t* base = c->d_pre.as<uint8_t>();
  HIPCHK(c, hipMemcpyAsync(base, in.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
  PreemptDev pe{};
  const auto bt = bound_dev(pe, c->d_bound.as<const uint8_t>(), c->blay);
  pe.bnviol = bt.nviol;
  pe.bstride = std::max<uint32_t>(c->bound_b, 1);
  pe.q = count;
  pe.nchunks = nchunks;
  pe.chunk_nodes = chunk_nodes;
  pe.cap = victim_cap;
  pe.spod = o_spod.in(base);
  pe.sprio = o_sprio.in(base);
  pe.sorig = o_sorig.in(base);
  pe.gprot = o_gprot.in(base);
  pe.r_node = o_rnode.in(base);
  pe.r_nv = o_rnv.in(base);
  pe.r_npv = o_rnpv.in(base);
  pe.r_top = o_rtop.in(base);
  pe.r_sum = o_rsum.in(base);
  pe.r_est = o_rest.in(base);
  pe.r_ncand = o_rncand.in(base);
  pe.o_node = o_node.in(base);
  pe.o_ncand = o_ncand.in(base);
  pe.o_nv = o_nv.in(base);
  pe.o_npv = o_npv.in(base);
  pe.o_top = o_top.in(base);
  pe.o_sum = o_sum.in(base);
  pe.o_est = o_est.in(base);
  pe.o_victims = o_vic.in(base);
  pe.nm = nom_view(c);
  launch_preempt(c->stream, c->S, dim3(tiles, nchunks), nodes_dev(c), pods_dev(c), pe);
  LAUNCHCHK(c, BS_KERNEL_QUERY);
  std::vector<uint8_t> res(cv.mark() - o_res);
  HIPCHK(c, hipMemcpyAsync(res.data(), base + o_res, res.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* rb = res.data() - o_res;
  std::memcpy(out->node, o_node.in(rb), o_node.bytes());
  std::memcpy(out->n_victims, o_nv.in(rb), o_nv.bytes());
  c->pre_npv.assign(o_npv.in(rb), o_npv.in(rb) + nQ);
  c->have_pre_npv = true;
  c->have_gang = false;
  c->have_pre_nom = false;
  if (out->n_candidates) std::memcpy(out->n_candidates, o_ncand.in(rb), o_ncand.bytes());
  if (out->top_priority) std::memcpy(out->top_priority, o_top.in(rb), o_top.bytes());
  if (out->priority_sum) std::memcpy(out->priority_sum, o_sum.in(rb), o_sum.bytes());
  if (out->earliest_start) std::memcpy(out->earliest_start, o_est.in(rb), o_est.bytes());
  if (victim_cap) {
    // rows are written up to min(n_victims, cap); the rest of a row is unspecified: zero it for the caller
    const uint32_t* nv = o_nv.in(rb);
    const uint32_t* vic = o_vic.in(rb);
    for (size_t q = 0; q < nQ; ++q) {
      const uint32_t k = std::min(nv[q], victim_cap);
      std::memcpy(out->victims + q * victim_cap, vic + q * victim_cap, (size_t)k * 4);
      std::memset(out->victims + q * victim_cap + k, 0, (size_t)(victim_cap - k) * 4);
    }
  }
  return BS_OK;
}

int bs_bound_load_flat(bs_ctx* c, uint32_t b, const uint32_t* node, const int32_t* priority, const int64_t* start_ns, const int32_t* group,
                       const int64_t* req, const uint32_t* req_present) {
  const bs_bound_soa bd{b, node, priority, start_ns, group, req, req_present};
  return bs_bound_load(c, &bd);
}

int bs_preempt_run_flat(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority, const uint8_t* group_protected,
                        uint32_t victim_cap, int32_t* node, uint32_t* n_candidates, uint32_t* n_victims, uint32_t* victims, int32_t* top_priority,
                        int64_t* priority_sum, int64_t* earliest_start) {
  const bs_preempt_out o{node, n_candidates, n_victims, victims, top_priority, priority_sum, earliest_start};
  return bs_preempt_run(c, stages, count, pod_index, priority, group_protected, victim_cap, &o);
}

// -------------------------------------------------------------------------------------------------
// preemption plans answered in sequence (bs_preempt_commit.hpp), applied into the resident state on request
// -------------------------------------------------------------------------------------------------
// bs_preempt_commit (gang == false: gang_need is not looked at, k_pc_resolve<S> is launched, the blob holds no gang column) and
// bs_preempt_commit_gang (gang == true: the run check on the sorted slots, k_gang_resolve<S>).  Validation, blob, scan launch, result
// copy and the APPLY tail are one code path.
static int preempt_commit_call(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority,
                               const uint8_t* group_protected, const uint32_t* gang_need, bool gang, uint32_t flags, uint32_t victim_cap,
                               const bs_preempt_out* out) {
  if (!c || !out) return BS_ERR_INVALID;
  if (stages & ~BS_STAGE_PREFILTER) { c->last_error = "bs_preempt_commit takes BS_STAGE_PREFILTER only (the plugin's Filter takes no part)"; return BS_ERR_INVALID; }
  if (flags & ~(BS_PREEMPT_APPLY | BS_PREEMPT_ASSUME | BS_PREEMPT_NOMINATE)) { c->last_error = "bs_preempt_commit: unknown flags"; return BS_ERR_INVALID; }
  if ((flags & BS_PREEMPT_ASSUME) && !(flags & BS_PREEMPT_APPLY)) { c->last_error = "BS_PREEMPT_ASSUME needs BS_PREEMPT_APPLY"; return BS_ERR_INVALID; }
  if ((flags & BS_PREEMPT_NOMINATE) && !(flags & BS_PREEMPT_APPLY)) { c->last_error = "BS_PREEMPT_NOMINATE needs BS_PREEMPT_APPLY"; return BS_ERR_INVALID; }
  if ((flags & BS_PREEMPT_NOMINATE) && (flags & BS_PREEMPT_ASSUME)) {
    c->last_error = "BS_PREEMPT_NOMINATE with BS_PREEMPT_ASSUME: the nominee would count twice";
    return BS_ERR_INVALID;
  }
  const bool nominate = (flags & BS_PREEMPT_NOMINATE) != 0;
  if (!c->have_nodes || !c->have_fit || !c->have_pods || !c->have_bound) {
    c->last_error = "bs_preempt_commit needs nodes, fit, pods and the bound table loaded";
    return BS_ERR_STATE;
  }
  if (c->nranks > 1 || c->reduce_external) { c->last_error = "bs_preempt_commit is single-rank only"; return BS_ERR_STATE; }
  if (c->bound_n != c->N) { c->last_error = "the bound table was loaded for another node list: reload it"; return BS_ERR_STATE; }
  if (const int nrc = nom_preempt_state(c, "bs_preempt_commit")) return nrc;
  if (nominate)
    if (const int nrc = nom_state(c, "BS_PREEMPT_NOMINATE")) return nrc;
  if (count > BS_PREEMPT_MAX || (uint64_t)count * victim_cap > (1ull << 28)) return BS_ERR_CAPACITY;
  if (nominate)                                           // against count, before any launch: all or nothing
    if (const int bad = nom_nominate_check(c->nom_w, c->nom_ids, count, BS_NOM_MAX, kNomMaxIds)) return nom_refusal(c, "BS_PREEMPT_NOMINATE", bad);
  if (gang && c->G && !gang_need) { c->last_error = "bs_preempt_commit_gang: gang_need is NULL with g > 0"; return BS_ERR_INVALID; }
  if (count == 0) {
    c->pre_npv.clear();
    c->have_pre_npv = true;
    c->have_gang = gang;
    if (gang) { c->gang_voided.clear(); c->gang_placed.assign(c->G, 0u); }
    c->pre_nom.clear();
    c->have_pre_nom = nominate;
    return BS_OK;
  }
  if (!pod_index || !priority || !out->node || !out->n_victims || (victim_cap && !out->victims) || (c->G && !group_protected)) return BS_ERR_INVALID;
  if (c->bound_max_group >= (int32_t)c->G) { c->last_error = "the bound table names a group index >= the loaded group count"; return BS_ERR_INVALID; }
  const uint32_t P = c->P, N = c->N, G = c->G, L = c->L, B = c->bound_b;
  for (uint32_t i = 0; i < count; ++i)
    if (pod_index[i] >= P) { c->last_error = "preemptor pod index >= p"; return BS_ERR_INVALID; }
  {
    std::vector<uint32_t> seen(pod_index, pod_index + count);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { c->last_error = "bs_preempt_commit: a pod index appears twice (a pod is nominated once)"; return BS_ERR_INVALID; }
  }
  const bool apply = (flags & BS_PREEMPT_APPLY) != 0, assume = (flags & BS_PREEMPT_ASSUME) != 0;
  int rc = use_device(c);
  if (rc) return rc;
  std::vector<uint32_t> perm(count);
  for (uint32_t i = 0; i < count; ++i) perm[i] = i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return priority[a] > priority[b]; });
  // gang: the runs of the sorted slots (bs_preempt_gang_runs.hpp).  The pods' group column lives on the device only (bs_pods_apply patches
  // it there), so it is read back when some group has a requirement; a second run of one group is refused before anything is launched.
  std::vector<uint32_t> g_need, g_rlen;
  std::vector<int32_t> sgroup;
  if (gang) {
    bool any = false;
    for (uint32_t g = 0; g < G; ++g) any |= gang_need[g] != 0;
    sgroup.assign(count, BS_POD_NOT_GROUPED);
    if (any) {
      std::vector<int32_t> pgroup(P);
      HIPCHK(c, hipMemcpyAsync(pgroup.data(), pods_dev(c).group, (size_t)P * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (uint32_t s = 0; s < count; ++s) sgroup[s] = pgroup[pod_index[perm[s]]];
    }
    if (gang_runs(count, sgroup.data(), G, gang_need, g_need, g_rlen) >= 0) {
      c->last_error = "bs_preempt_commit_gang: a group with a requirement forms more than one run of slots";
      return BS_ERR_INVALID;
    }
  }
  if (apply && (rc = settle_pending(c))) return rc;
  const PreemptGeom geom = preempt_geom(N, count, c->test_pc_chunk_nodes);   // slot tiles x node chunks (bs_preempt_geom.hpp)
  const uint32_t tiles = geom.tiles, nchunks = geom.nchunks, chunk_nodes = geom.chunk_nodes;
  const size_t nQ = count, nG = std::max<uint32_t>(G, 1), nR = (size_t)nchunks * nQ, nV = std::max<size_t>((size_t)nQ * victim_cap, 1);
  const size_t nN = std::max<uint32_t>(N, 1), nB = std::max<uint32_t>(B, 1);
  Carve cv;
  const auto o_spod = cv.take<uint32_t>(nQ);
  const auto o_sprio = cv.take<int32_t>(nQ);
  const auto o_sorig = cv.take<uint32_t>(nQ);
  const auto o_gprot = cv.take<uint8_t>(nG);
  const size_t gQ = gang ? nQ : 0, gB = gang ? nB : 0;    // gang columns: no bytes in bs_preempt_commit's blob
  const auto o_gneed = cv.take<uint32_t>(gQ);
  const auto o_grlen = cv.take<uint32_t>(gQ);
  const size_t in_bytes = cv.mark();
  const auto o_rnode = cv.take<int32_t>(nR * kPcK);
  const auto o_rnv = cv.take<uint32_t>(nR * kPcK);
  const auto o_rnpv = cv.take<uint32_t>(nR * kPcK);
  const auto o_rtop = cv.take<int32_t>(nR * kPcK);
  const auto o_rsum = cv.take<int64_t>(nR * kPcK);
  const auto o_rest = cv.take<int64_t>(nR * kPcK);
  const auto o_rncand = cv.take<uint32_t>(nR);
  const size_t o_work = cv.mark();                          // zeroed working state
  const auto o_dv = cv.take<int64_t>((size_t)L * nN);
  const auto o_dn = cv.take<int64_t>((size_t)L * nN);
  const auto o_vbits = cv.take<uint32_t>(nN);
  const auto o_nbits = cv.take<uint32_t>(nN);
  const auto o_dirty = cv.take<uint8_t>(nN);
  const auto o_dead = cv.take<uint8_t>(nB);
  const auto o_gtag = cv.take<uint32_t>(gB);
  const auto o_gplaced = cv.take<uint32_t>(gQ);
  const auto o_gvoided = cv.take<uint8_t>(gQ);
  const size_t work_bytes = cv.mark() - o_work;
  const auto o_gslog = cv.take<uint32_t>(gQ * 3);
  const auto o_dlist = cv.take<uint32_t>(nQ);
  const auto o_nreq = cv.take<bs_node_request>(nQ);
  const size_t o_res = cv.mark();                           // results: one D2H
  const auto o_info = cv.take<uint32_t>(2);
  const auto o_node = cv.take<int32_t>(nQ);
  const auto o_ncand = cv.take<uint32_t>(nQ);
  const auto o_nv = cv.take<uint32_t>(nQ);
  const auto o_npv = cv.take<uint32_t>(nQ);
  const auto o_top = cv.take<int32_t>(nQ);
  const auto o_sum = cv.take<int64_t>(nQ);
  const auto o_est = cv.take<int64_t>(nQ);
  const auto o_vic = cv.take<uint32_t>(nV);
  HIPCHK(c, c->d_pre.reserve(cv.mark()));
  std::vector<uint8_t> in(in_bytes, 0);
  for (uint32_t s = 0; s < count; ++s) {
    o_spod.in(in.data())[s] = pod_index[perm[s]];
    o_sprio.in(in.data())[s] = priority[perm[s]];
    o_sorig.in(in.data())[s] = perm[s];
  }
  if (G) std::memcpy(o_gprot.in(in.data()), group_protected, G);
  if (gang) {
    std::memcpy(o_gneed.in(in.data()), g_need.data(), o_gneed.bytes());
    std::memcpy(o_grlen.in(in.data()), g_rlen.data(), o_grlen.bytes());
  }
  uint8_t* base = c->d_pre.as<uint8_t>();
  HIPCHK(c, hipMemcpyAsync(base, in.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(base + o_work, 0, work_bytes, c->stream));
  CommitDev pe{};
  const auto bt = bound_dev(pe, c->d_bound.as<const uint8_t>(), c->blay);
  pe.bpres = bt.pres;
  pe.bnviol = bt.nviol;
  pe.bstride = (uint32_t)nB;
  pe.q = count;
  pe.nchunks = nchunks;
  pe.chunk_nodes = chunk_nodes;
  pe.cap = victim_cap;
  pe.spod = o_spod.in(base);
  pe.sprio = o_sprio.in(base);
  pe.sorig = o_sorig.in(base);
  pe.gprot = o_gprot.in(base);
  pe.r_node = o_rnode.in(base);
  pe.r_nv = o_rnv.in(base);
  pe.r_npv = o_rnpv.in(base);
  pe.r_top = o_rtop.in(base);
  pe.r_sum = o_rsum.in(base);
  pe.r_est = o_rest.in(base);
  pe.r_ncand = o_rncand.in(base);
  pe.dv = o_dv.in(base);
  pe.dn = o_dn.in(base);
  pe.vbits = o_vbits.in(base);
  pe.nbits = o_nbits.in(base);
  pe.dirty = o_dirty.in(base);
  pe.dead = o_dead.in(base);
  pe.dlist = o_dlist.in(base);
  pe.info = o_info.in(base);
  pe.o_node = o_node.in(base);
  pe.o_ncand = o_ncand.in(base);
  pe.o_nv = o_nv.in(base);
  pe.o_npv = o_npv.in(base);
  pe.o_top = o_top.in(base);
  pe.o_sum = o_sum.in(base);
  pe.o_est = o_est.in(base);
  pe.o_victims = o_vic.in(base);
  pe.nm = nom_view(c);
  const NodesDev nd = nodes_dev(c);
  if (gang) {
    GangDev gd{};
    gd.s_need = o_gneed.in(base);
    gd.s_rlen = o_grlen.in(base);
    gd.tag = o_gtag.in(base);
    gd.slog = o_gslog.in(base);
    gd.o_placed = o_gplaced.in(base);
    gd.o_voided = o_gvoided.in(base);
    launch_preempt_commit_gang(c->stream, c->S, dim3(tiles, nchunks), nd, pods_dev(c), pe, gd);
  } else {
    launch_preempt_commit(c->stream, c->S, dim3(tiles, nchunks), nd, pods_dev(c), pe);
  }
  LAUNCHCHK(c, BS_KERNEL_QUERY);
  std::vector<uint8_t> res(cv.mark() - o_res);
  HIPCHK(c, hipMemcpyAsync(res.data(), base + o_res, res.size(), hipMemcpyDeviceToHost, c->stream));
  std::vector<uint8_t> gres;                              // gang: placed by slot, then voided by preemptor (adjacent in the blob)
  if (gang) {
    gres.resize(o_work + work_bytes - o_gplaced.off);
    HIPCHK(c, hipMemcpyAsync(gres.data(), o_gplaced.in(base), gres.size(), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* rb = res.data() - o_res;
  if (apply) {
    const uint32_t* info = o_info.in(rb);
    const uint32_t ndirty = info[0], nvall = info[1];
    bs_node_request* dreq = o_nreq.in(base);
    CompactDev nw{};
    const uint32_t B2 = B - nvall;
    BoundLayout lay{};
    if (nvall) {                                          // the compacted table goes to the second buffer, swapped in below
      HIPCHK(c, c->d_bound2.reserve(bound_layout(L, N, B2, lay)));
      const auto nt = bound_dev(nw, c->d_bound2.as<uint8_t>(), lay);
      nw.bpres = nt.pres;
      nw.bnviol = nt.nviol;
      nw.bstride = std::max<uint32_t>(B2, 1);
    }
    launch_preempt_apply(c->stream, c->S, nd, pe, ndirty, assume ? 1u : 0u, dreq, nvall ? &nw : nullptr);
    LAUNCHCHK(c, BS_KERNEL_QUERY);
    if (ndirty) {
      launch_nodes_assume(c, dreq, ndirty);
      LAUNCHCHK(c, BS_KERNEL_PREPASS);
      std::vector<bs_node_request> h(ndirty);
      HIPCHK(c, hipMemcpyAsync(h.data(), dreq, (size_t)ndirty * sizeof(bs_node_request), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      mirror_node_requests(c, h.data(), ndirty);
      c->bitmap_valid = false;
    }
    if (nvall) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      std::swap(c->d_bound.p, c->d_bound2.p);
      std::swap(c->d_bound.cap, c->d_bound2.cap);
      c->blay = lay;
      c->bound_b = B2;
    }
  }
  if (nominate) {
    // every slot that holds a node (gang: not voided, its node is -1 otherwise) is appended to the table, in the caller's order
    const int32_t* rnode = o_node.in(rb);
    std::vector<uint32_t> npod, nnode;
    std::vector<int32_t> nprio;
    c->pre_nom.assign(nQ, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < count; ++i)
      if (rnode[i] >= 0) {
        c->pre_nom[i] = c->nom_ids + (uint32_t)npod.size();
        npod.push_back(pod_index[i]);
        nnode.push_back((uint32_t)rnode[i]);
        nprio.push_back(priority[i]);
      }
    if (!npod.empty() && (rc = nom_apply_rows(c, 0u, nullptr, (uint32_t)npod.size(), npod.data(), nnode.data(), nprio.data()))) return rc;
  }
  c->have_pre_nom = nominate;
  std::memcpy(out->node, o_node.in(rb), o_node.bytes());
  std::memcpy(out->n_victims, o_nv.in(rb), o_nv.bytes());
  c->pre_npv.assign(o_npv.in(rb), o_npv.in(rb) + nQ);
  c->have_pre_npv = true;
  c->have_gang = gang;
  if (gang) {
    const uint32_t* placed = o_gplaced.in(gres.data() - o_gplaced.off);
    const uint8_t* voided = o_gvoided.in(gres.data() - o_gplaced.off);
    c->gang_voided.assign(voided, voided + nQ);
    c->gang_placed.assign(G, 0u);
    for (uint32_t s = 0; s < count; ++s)
      if (g_rlen[s]) c->gang_placed[sgroup[s]] = placed[s];
  }
  if (out->n_candidates) std::memcpy(out->n_candidates, o_ncand.in(rb), o_ncand.bytes());
  if (out->top_priority) std::memcpy(out->top_priority, o_top.in(rb), o_top.bytes());
  if (out->priority_sum) std::memcpy(out->priority_sum, o_sum.in(rb), o_sum.bytes());
  if (out->earliest_start) std::memcpy(out->earliest_start, o_est.in(rb), o_est.bytes());
  if (victim_cap) {
    const uint32_t* nv = o_nv.in(rb);
    const uint32_t* vic = o_vic.in(rb);
    for (size_t q = 0; q < nQ; ++q) {
      const uint32_t k = std::min(nv[q], victim_cap);
      std::memcpy(out->victims + q * victim_cap, vic + q * victim_cap, (size_t)k * 4);
      std::memset(out->victims + q * victim_cap + k, 0, (size_t)(victim_cap - k) * 4);
    }
  }
  return BS_OK;
}

int bs_preempt_commit(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority, const uint8_t* group_protected,
                      uint32_t flags, uint32_t victim_cap, const bs_preempt_out* out) {
  return preempt_commit_call(c, stages, count, pod_index, priority, group_protected, nullptr, false, flags, victim_cap, out);
}

int bs_preempt_commit_gang(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority,
                           const uint8_t* group_protected, const uint32_t* gang_need, uint32_t flags, uint32_t victim_cap, const bs_preempt_out* out) {
  return preempt_commit_call(c, stages, count, pod_index, priority, group_protected, gang_need, true, flags, victim_cap, out);
}

int bs_preempt_gang_read(bs_ctx* c, uint32_t count, uint8_t* slot_voided, uint32_t g, uint32_t* group_placed) {
  if (!c) return BS_ERR_INVALID;
  if (!c->have_gang) { c->last_error = "bs_preempt_gang_read: the last preemption call was not a successful bs_preempt_commit_gang"; return BS_ERR_STATE; }
  if (count != c->gang_voided.size() || g != c->gang_placed.size()) {
    c->last_error = "bs_preempt_gang_read: count or g differ from the last bs_preempt_commit_gang's";
    return BS_ERR_INVALID;
  }
  if (slot_voided && count) std::memcpy(slot_voided, c->gang_voided.data(), count);
  if (group_placed && g) std::memcpy(group_placed, c->gang_placed.data(), (size_t)g * 4);
  return BS_OK;
}

int bs_bound_read(bs_ctx* c, uint32_t* id_out, uint32_t* node_out) {
  if (!c) return BS_ERR_INVALID;
  if (!c->have_bound) { c->last_error = "bs_bound_read before bs_bound_load"; return BS_ERR_STATE; }
  const uint32_t B = c->bound_b, N = c->bound_n;
  if (B == 0) return BS_OK;
  if (!id_out || !node_out) return BS_ERR_INVALID;
  int rc = use_device(c);
  if (rc) return rc;
  std::vector<uint32_t> boff((size_t)N + 1);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const auto bt = bound_cols(c->d_bound.as<const uint8_t>(), c->blay);
  HIPCHK(c, hipMemcpy(boff.data(), bt.boff, ((size_t)N + 1) * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(id_out, bt.id, (size_t)B * 4, hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < N; ++k)
    for (uint32_t j = boff[k]; j < boff[k + 1] && j < B; ++j) node_out[j] = k;
  return BS_OK;
}

// -------------------------------------------------------------------------------------------------
// the bound table patched in place (bs_bound_apply.hpp): O(delta) on the host, one pass over the table on the device
// -------------------------------------------------------------------------------------------------
int bs_bound_ids(const bs_ctx* c, uint32_t* ids_out) {
  if (!c || !ids_out) return BS_ERR_INVALID;
  *ids_out = c->have_bound ? c->bound_ids : 0u;
  return BS_OK;
}

// flags: 0 = bs_bound_apply; BS_BOUND_NODES = the node requests follow (bs_bound_apply_ex)
static int bound_apply(bs_ctx* c, const bs_bound_delta* d, uint32_t flags, uint32_t* first_id_out) {
  if (!c || !d) return BS_ERR_INVALID;
  if (flags & ~BS_BOUND_NODES) { c->last_error = "bs_bound_apply_ex: unknown flags"; return BS_ERR_INVALID; }
  const bool with_nodes = (flags & BS_BOUND_NODES) != 0;
  if (!c->have_bound) { c->last_error = "bs_bound_apply before bs_bound_load"; return BS_ERR_STATE; }
  if (with_nodes && !c->have_nodes) { c->last_error = "bs_bound_apply_ex(BS_BOUND_NODES) before bs_nodes_load"; return BS_ERR_STATE; }
  if (c->bound_n != c->N) { c->last_error = "the bound table was loaded for another node list: reload it"; return BS_ERR_STATE; }
  const uint32_t R = d->n_remove, I = d->n_insert, N = c->N, L = c->L, B = c->bound_b, ids = c->bound_ids;
  if (R && !d->remove) return BS_ERR_INVALID;
  if (I && (!d->node || !d->priority || !d->start_ns || !d->group || !d->req || !d->req_present)) return BS_ERR_INVALID;
  if (R == 0 && I == 0) {
    if (first_id_out) *first_id_out = ids;
    return BS_OK;
  }
  int32_t gmax = c->bound_max_group;
  for (uint32_t i = 0; i < I; ++i) {
    if (d->node[i] >= N) { c->last_error = "bs_bound_apply: insert on a node index >= n"; return BS_ERR_INVALID; }
    if (d->group[i] < BS_POD_GROUP_MISSING) { c->last_error = "bs_bound_apply: insert group index below BS_POD_GROUP_MISSING"; return BS_ERR_INVALID; }
    gmax = std::max(gmax, d->group[i]);
  }
  for (uint32_t r = 0; r < R; ++r)
    if (d->remove[r] >= ids) { c->last_error = "bs_bound_apply: remove id outside the id space"; return BS_ERR_INVALID; }
  if (R > B) { c->last_error = "bs_bound_apply: more remove ids than live entries (an id is listed twice or is not live)"; return BS_ERR_INVALID; }
  if ((uint64_t)ids + I > BS_BOUND_MAX) { c->last_error = "bs_bound_apply: the id space would pass BS_BOUND_MAX: reload the table"; return BS_ERR_CAPACITY; }
  int rc = use_device(c);
  if (rc) return rc;
  if (with_nodes && (rc = settle_pending(c))) return rc;   // as bs_nodes_assume: a pending batch is settled against the state it was launched on
  // the inserts by (node, importance); their ids follow the delta's order, so equal keys keep it
  std::vector<uint32_t> order(I);
  for (uint32_t i = 0; i < I; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (d->node[a] != d->node[b]) return d->node[a] < d->node[b];
    if (d->priority[a] != d->priority[b]) return d->priority[a] > d->priority[b];
    if (d->start_ns[a] != d->start_ns[b]) return d->start_ns[a] < d->start_ns[b];
    return a < b;
  });
  // one blob (8-byte columns first), then the scratch: pos_of (0xff), the zeroed words, the segment starts
  const size_t nI = I, nR = R, nN = std::max<uint32_t>(N, 1);
  Carve cv;
  const auto o_start = cv.take<int64_t>(nI, 1);           // (packed)
  const auto o_req = cv.take<int64_t>(nI * L, 1);
  const auto o_rem = cv.take<uint32_t>(nR, 1);
  const auto o_node = cv.take<uint32_t>(nI, 1);
  const auto o_prio = cv.take<int32_t>(nI, 1);
  const auto o_group = cv.take<int32_t>(nI, 1);
  const auto o_id = cv.take<uint32_t>(nI, 1);
  const auto o_pres = cv.take<uint32_t>(nI, 1);
  const auto o_pdb = cv.take<uint8_t>(nI);                 // the last column: the scratch behind it starts at the next 256
  const size_t blob_bytes = o_pdb.off + o_pdb.bytes();
  const auto o_posof = cv.take<uint32_t>(std::max<uint32_t>(ids, 1));
  const size_t o_zero = cv.mark();
  const auto o_deadw = cv.take<uint32_t>((size_t)B / 32 + 1);
  const auto o_dcnt = cv.take<uint32_t>(nN);
  const auto o_icnt = cv.take<uint32_t>(nN);
  const auto o_err = cv.take<uint32_t>(1);
  const auto o_gap = cv.take<uint8_t>(256);
  const Piece<uint32_t> o_nrec{o_gap.off + 248, 2};        // BS_BOUND_NODES: the record count, the last 8 bytes before the records (one D2H)
  const size_t zero_bytes = cv.mark() - o_zero;
  const size_t rec_cap = with_nodes ? std::min<size_t>(N, nR + nI) : 0;
  const auto o_rec = cv.take<bs_node_request>(rec_cap);
  const auto o_ifirst = cv.take<uint32_t>(nN);
  // the id space grows with every call, and the table with every net insert: a quarter of headroom, so that a run of calls allocates rarely
  if (cv.mark() > c->d_pre.cap) HIPCHK(c, c->d_pre.reserve(cv.mark() + cv.mark() / 4));
  std::vector<uint8_t> h(std::max<size_t>(blob_bytes, 1), 0);
  uint8_t* hb = h.data();
  if (R) std::memcpy(o_rem.in(hb), d->remove, o_rem.bytes());
  const uint32_t smask = (uint32_t)((1ull << (L - BS_FIXED_LANES)) - 1ull);
  for (uint32_t r = 0; r < I; ++r) {                       // stored as bs_bound_load stores them
    const uint32_t i = order[r];
    o_node.in(hb)[r] = d->node[i];
    o_prio.in(hb)[r] = d->priority[i];
    o_start.in(hb)[r] = d->start_ns[i];
    o_group.in(hb)[r] = d->group[i];
    o_id.in(hb)[r] = ids + i;
    o_pres.in(hb)[r] = d->req_present[i] & smask;
    o_pdb.in(hb)[r] = d->pdb_violating && d->pdb_violating[i] ? 1 : 0;
    for (uint32_t l = 0; l < L; ++l) {
      int64_t v = d->req[(size_t)l * I + i];
      if (l == BS_LANE_PODS) v = 1;
      else if (l >= BS_FIXED_LANES && !((d->req_present[i] >> (l - BS_FIXED_LANES)) & 1u)) v = 0;
      o_req.in(hb)[(size_t)l * nI + r] = v;
    }
  }
  uint8_t* base = c->d_pre.as<uint8_t>();
  HIPCHK(c, hipMemcpyAsync(base, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(o_posof.in(base), 0xff, o_posof.bytes(), c->stream));
  HIPCHK(c, hipMemsetAsync(base + o_zero, 0, zero_bytes, c->stream));
  BoundApplyDev a{};
  a.n_remove = R; a.n_insert = I;
  a.rem = o_rem.in(base);
  a.inode = o_node.in(base);
  a.iprio = o_prio.in(base);
  a.istart = o_start.in(base);
  a.igroup = o_group.in(base);
  a.ireq = o_req.in(base);
  a.iid = o_id.in(base);
  a.ipres = o_pres.in(base);
  a.ipdb = o_pdb.in(base);
  a.pos_of = o_posof.in(base);
  a.deadw = o_deadw.in(base);
  a.dcnt = o_dcnt.in(base);
  a.icnt = o_icnt.in(base);
  a.ifirst = o_ifirst.in(base);
  a.err = o_err.in(base);
  if ((rc = bound_apply_block(c, "bs_bound_apply", a, gmax))) return rc;
  if (first_id_out) *first_id_out = ids;
  if (with_nodes && rec_cap) {
    // the node requests follow: `a` still names the old table (now the second allocation, intact) and the scratch k_ba_mark left
    BoundNodesReqDev o2{};
    o2.nreq = c->d_nreq.as<int64_t>();
    o2.rpres = c->d_rpres.as<uint32_t>();
    o2.nstride = c->Ncap;
    o2.cap = (uint32_t)rec_cap;
    o2.count = o_nrec.in(base);
    o2.out = o_rec.in(base);
    launch_bound_apply_nodes(c->stream, c->S, a, o2);
    LAUNCHCHK(c, BS_KERNEL_PREPASS);
    std::vector<uint8_t> hr(8 + rec_cap * sizeof(bs_node_request));   // count + records
    HIPCHK(c, hipMemcpyAsync(hr.data(), o_nrec.in(base), hr.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint32_t nrec = 0;
    std::memcpy(&nrec, hr.data(), 4);
    if (nrec > rec_cap) { c->last_error = "bs_bound_apply_ex: more touched nodes than the delta can touch"; return BS_ERR_HIP; }
    if (nrec) {
      launch_nodes_assume(c, o2.out, nrec);
      LAUNCHCHK(c, BS_KERNEL_PREPASS);
      mirror_node_requests(c, reinterpret_cast<const bs_node_request*>(hr.data() + 8), nrec);
      c->bitmap_valid = false;
    }
  }
  return BS_OK;
}

int bs_bound_apply(bs_ctx* c, const bs_bound_delta* d, uint32_t* first_id_out) { return bound_apply(c, d, 0u, first_id_out); }

int bs_bound_apply_ex(bs_ctx* c, const bs_bound_delta* d, uint32_t flags, uint32_t* first_id_out) { return bound_apply(c, d, flags, first_id_out); }

int bs_bound_apply_ex_flat(bs_ctx* c, uint32_t flags, uint32_t n_remove, const uint32_t* remove, uint32_t n_insert, const uint32_t* node,
                           const int32_t* priority, const int64_t* start_ns, const int32_t* group, const int64_t* req, const uint32_t* req_present,
                           const uint8_t* pdb_violating, uint32_t* first_id_out) {
  const bs_bound_delta d{n_remove, remove, n_insert, node, priority, start_ns, group, req, req_present, pdb_violating};
  return bound_apply(c, &d, flags, first_id_out);
}

int bs_bound_apply_flat(bs_ctx* c, uint32_t n_remove, const uint32_t* remove, uint32_t n_insert, const uint32_t* node, const int32_t* priority,
                        const int64_t* start_ns, const int32_t* group, const int64_t* req, const uint32_t* req_present, const uint8_t* pdb_violating,
                        uint32_t* first_id_out) {
  const bs_bound_delta d{n_remove, remove, n_insert, node, priority, start_ns, group, req, req_present, pdb_violating};
  return bs_bound_apply(c, &d, first_id_out);
}

// -------------------------------------------------------------------------------------------------
// the bound table follows node-list surgery (bs_bound_nodes.hpp): O(count) on the host, one pass over the table on the device
// -------------------------------------------------------------------------------------------------
int bs_bound_nodes_apply(bs_ctx* c, uint32_t count, const uint32_t* kind, const uint32_t* index, uint32_t dropped_cap, uint32_t* dropped_ids,
                         uint32_t* n_dropped_out) {
  if (!c) return BS_ERR_INVALID;
  if (!c->have_bound) { c->last_error = "bs_bound_nodes_apply before bs_bound_load"; return BS_ERR_STATE; }
  if (c->nranks > 1 || c->reduce_external) { c->last_error = "bs_bound_nodes_apply is single-rank only"; return BS_ERR_STATE; }
  if ((count && (!kind || !index)) || (dropped_cap && !dropped_ids)) return BS_ERR_INVALID;
  const uint32_t N0 = c->bound_n, L = c->L, B = c->bound_b;
  NodeReplay rp;
  if (bound_nodes_replay(N0, count, kind, index, rp)) {
    c->last_error = "bs_bound_nodes_apply: a kind outside UPDATE / APPEND / REMOVE, or an index at or beyond the node count at its point of the replay";
    return BS_ERR_INVALID;
  }
  if (rp.n_new != c->N) { c->last_error = "bs_bound_nodes_apply: the replay does not end at the node count: not the list bs_nodes_apply got"; return BS_ERR_STATE; }
  const uint32_t N1 = rp.n_new, R = (uint32_t)rp.removed.size();
  if (R == 0 && rp.appended == 0) {                        // updates, or appends removed again: the table stays as it is
    if (n_dropped_out) *n_dropped_out = 0;
    return BS_OK;
  }
  int rc = use_device(c);
  if (rc) return rc;
  // the removed list (one H2D), then the scratch of this call
  const uint32_t nblk = std::max<uint32_t>(1u, cdiv(std::max(N1, R), 1024u)), ncap = std::min(dropped_cap, B);
  const size_t nR = R, nN = N1;
  Carve cv;
  const auto o_rem = cv.take<uint32_t>(nR);
  const auto o_len = cv.take<uint32_t>(nN);
  const auto o_src = cv.take<uint32_t>(nN);
  const auto o_dlen = cv.take<uint32_t>(nR);
  const auto o_doff = cv.take<uint32_t>(nR + 1);
  const auto o_bsum = cv.take<uint32_t>((size_t)2 * nblk);
  const auto o_pair = cv.take<uint32_t>(2);
  const auto o_drop = cv.take<uint32_t>(ncap);
  if (cv.mark() > c->d_pre.cap) HIPCHK(c, c->d_pre.reserve(cv.mark() + cv.mark() / 4));
  // the new table holds at most the old entries: sized for them, laid out by k_bn_move for the count the scan finds (boff: N1 + 1 words,
  // nviol: N1 words — appends grow both)
  BoundLayout lay{};
  const size_t table_bytes = bound_layout(L, N1, B, lay);
  if (table_bytes > c->d_bound2.cap) HIPCHK(c, c->d_bound2.reserve(table_bytes + table_bytes / 4));
  uint8_t* base = c->d_pre.as<uint8_t>();
  if (R) HIPCHK(c, hipMemcpyAsync(o_rem.in(base), rp.removed.data(), o_rem.bytes(), hipMemcpyHostToDevice, c->stream));
  BoundNodesDev a{};
  const auto bt = bound_dev(a, c->d_bound.as<const uint8_t>(), c->blay);
  a.bpres = bt.pres;
  a.bstride = std::max<uint32_t>(B, 1);
  a.n0 = N0; a.n1 = N1;
  a.nrem = R; a.old_left = N0 - R;
  a.rem = o_rem.in(base);
  a.nbase = c->d_bound2.as<uint8_t>();
  a.nboff = bound_cols(a.nbase, lay).boff;
  a.len = o_len.in(base);
  a.src = o_src.in(base);
  a.dlen = o_dlen.in(base);
  a.doff = o_doff.in(base);
  a.bsum = o_bsum.in(base);
  a.nblk = nblk;
  a.pair = o_pair.in(base);
  a.dropped = o_drop.in(base);
  a.dropped_cap = ncap;
  launch_bound_nodes(c->stream, c->S, a);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  uint32_t pair[2] = {0, 0};                               // {new entry count, dropped count}: read before the swap
  HIPCHK(c, hipMemcpyAsync(pair, a.pair, o_pair.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));              // (rp.removed and pair are local buffers)
  if ((uint64_t)pair[0] + pair[1] != B) { c->last_error = "bs_bound_nodes_apply: the resident table's offsets do not add up"; return BS_ERR_HIP; }
  const uint32_t nd = std::min(pair[1], ncap);
  if (nd) HIPCHK(c, hipMemcpy(dropped_ids, a.dropped, (size_t)nd * 4, hipMemcpyDeviceToHost));
  std::swap(c->d_bound.p, c->d_bound2.p);
  std::swap(c->d_bound.cap, c->d_bound2.cap);
  bound_layout(L, N1, pair[0], lay);                       // as k_bn_move laid it out
  c->blay = lay;
  c->bound_b = pair[0];
  c->bound_n = N1;
  if (n_dropped_out) *n_dropped_out = pair[1];
  return BS_OK;
}

int bs_bound_dump(bs_ctx* c, int32_t* priority, int64_t* start_ns, int32_t* group, int64_t* req, uint32_t* req_present, uint8_t* pdb) {
  if (!c) return BS_ERR_INVALID;
  if (!c->have_bound) { c->last_error = "bs_bound_dump before bs_bound_load"; return BS_ERR_STATE; }
  const size_t B = c->bound_b;
  if (B == 0) return BS_OK;
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const auto bt = bound_cols(c->d_bound.as<const uint8_t>(), c->blay);
  if (priority) HIPCHK(c, hipMemcpy(priority, bt.prio, B * 4, hipMemcpyDeviceToHost));
  if (start_ns) HIPCHK(c, hipMemcpy(start_ns, bt.start, B * 8, hipMemcpyDeviceToHost));
  if (group) HIPCHK(c, hipMemcpy(group, bt.group, B * 4, hipMemcpyDeviceToHost));
  if (req) HIPCHK(c, hipMemcpy(req, bt.req, B * c->L * 8, hipMemcpyDeviceToHost));   // the lane stride is the entry count
  if (req_present) HIPCHK(c, hipMemcpy(req_present, bt.pres, B * 4, hipMemcpyDeviceToHost));
  if (pdb) HIPCHK(c, hipMemcpy(pdb, bt.pdb, B, hipMemcpyDeviceToHost));
  return BS_OK;
}

int bs_preempt_commit_flat(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority, const uint8_t* group_protected,
                           uint32_t flags, uint32_t victim_cap, int32_t* node, uint32_t* n_candidates, uint32_t* n_victims, uint32_t* victims,
                           int32_t* top_priority, int64_t* priority_sum, int64_t* earliest_start) {
  const bs_preempt_out o{node, n_candidates, n_victims, victims, top_priority, priority_sum, earliest_start};
  return bs_preempt_commit(c, stages, count, pod_index, priority, group_protected, flags, victim_cap, &o);
}

int bs_preempt_commit_gang_flat(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority,
                                const uint8_t* group_protected, const uint32_t* gang_need, uint32_t flags, uint32_t victim_cap, int32_t* node,
                                uint32_t* n_candidates, uint32_t* n_victims, uint32_t* victims, int32_t* top_priority, int64_t* priority_sum,
                                int64_t* earliest_start) {
  const bs_preempt_out o{node, n_candidates, n_victims, victims, top_priority, priority_sum, earliest_start};
  return bs_preempt_commit_gang(c, stages, count, pod_index, priority, group_protected, gang_need, flags, victim_cap, &o);
}
}  // extern "C"
