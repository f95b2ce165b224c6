// tu_nominated.hip — translation unit of the resident nominated-pod table: pods nominated by earlier cycles, counted by every fit test of the
// victim search.  Kernels (bs_nominated.hpp): k_nm_mark and k_nm_chains (no templates: this unit alone includes that header), k_nm_move<S>,
// k_nm_gather<S> and k_nn_move<S> (the table follows node-list surgery), once per scalar-lane count 0..BS_MAX_SCALARS, and k_nc_list (the
// rows a BS_PREEMPT_CLEAR_LOWER plan cleared; no lanes).  Host: the table's
// layout, its file-local launch wrappers, the entry points bs_nominated_* (include/bsched.h), and what the preemption calls of
// tu_preempt.hip use the table through (bs_ctx.hpp): nom_view, nom_state, nom_preempt_state, nom_refusal, nom_apply_rows, nom_clear_list;
// and what the sequential pass of bs_seq_run_nominated (tu_seq.hip) takes its consumed rows off the table with: nom_drop_flagged.
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_nominated.hpp"
#include "bs_nominated_check.hpp"
#include "bs_nominated_nodes_check.hpp"
#include "bs_ctx.hpp"

#include <cstring>
#include <iterator>

namespace {

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
// the table follows node-list surgery: k_nn_move<S> (one workgroup); the chains follow (launch_nom_chains)
void launch_nom_nodes(hipStream_t stream, uint32_t S, const NomNodesDev& a) {
  lanes_wide(S, [&](auto s) { hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nn_move<decltype(s)::value>), dim3(1), dim3(kNmWindow), 0, stream, a); });
}
int nom_single_rank(bs_ctx* c, const char* who) {
  if (c->nranks > 1 || c->reduce_external) { c->last_error = std::string(who) + " is single-rank only (as bs_preempt_run)"; return BS_ERR_STATE; }
  return BS_OK;
}

}  // namespace

// what the victim search reads: null without a table or without rows (the callers have refused a stale table that holds rows)
const NomView* bs::nom_view(const bs_ctx* c) {
  if (!c->have_nom || c->nom_w == 0) return nullptr;
  const uint32_t cur = c->nom_cur;
  return nom_layout(c->nom_cap[cur], c->nom_ncap[cur], c->L).view.in((const void*)c->d_nom[cur].p);
}
// the table exists and was made for the node count the context holds now
int bs::nom_state(bs_ctx* c, const char* who) {
  if (const int rc = nom_single_rank(c, who)) return rc;
  if (!c->have_nom) { c->last_error = std::string(who) + ": no nominated-pod table (bs_nominated_load first; m = 0 gives the empty one)"; return BS_ERR_STATE; }
  if (!c->have_nodes || c->nom_n != c->N) {
    c->last_error = std::string(who) + ": the nominated-pod table was made for another node count (after node-list surgery: bs_nominated_nodes_apply; else bs_nominated_load)";
    return BS_ERR_STATE;
  }
  return BS_OK;
}
// what the three preemption calls refuse: rows of a table that was made for another node count
int bs::nom_preempt_state(bs_ctx* c, const char* who) {
  if (c->have_nom && c->nom_w && c->nom_n != c->N) {
    c->last_error = std::string(who) + ": the nominated-pod table holds rows and was made for another node count (after node-list surgery: bs_nominated_nodes_apply; else bs_nominated_load)";
    return BS_ERR_STATE;
  }
  return BS_OK;
}
int bs::nom_refusal(bs_ctx* c, const char* who, int bad) {
  c->last_error = std::string(who) + ": " + nom_check_text(bad);
  return nom_check_is_capacity(bad) ? BS_ERR_CAPACITY : BS_ERR_INVALID;
}
// k_nc_list behind a BS_PREEMPT_CLEAR_LOWER resolve (the caller has found the table live and with rows: its nom_view was not null)
void bs::nom_clear_list(bs_ctx* c, const uint32_t* thr, const uint32_t* first, const uint32_t* sorig, uint32_t* cols, uint32_t* count) {
  const size_t rows = std::max<uint32_t>(c->nom_w, 1);
  NomClearDev a{};
  a.src = nom_tab(c, c->nom_cur);
  a.W = c->nom_w;
  a.N = c->N;
  a.thr = thr;
  a.first = first;
  a.sorig = sorig;
  a.o_id = cols;
  a.o_node = cols + rows;
  a.o_prio = reinterpret_cast<int32_t*>(cols + 2 * rows);
  a.o_by = cols + 3 * rows;
  a.o_count = count;
  hipLaunchKernelGGL(k_nc_list, dim3(1), dim3(kNmWindow), 0, c->stream, a);
}
// bs_nominated_apply behind its checks (and BS_PREEMPT_NOMINATE's append): the listed rows leave by the stable compaction into the twin,
// the inserts are gathered from the resident queue behind the survivors, the chains are rebuilt, the twin becomes the table.  One wait.
int bs::nom_apply_rows(bs_ctx* c, uint32_t R, const uint32_t* remove_id, uint32_t I, const uint32_t* pod_index, const uint32_t* node,
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

// the sequential pass consumed rows (rule S): flag[] is the pass's own device array over the live table's rows, `gone` the same rows' ids
int bs::nom_drop_flagged(bs_ctx* c, const uint8_t* flag, const std::vector<uint32_t>& gone) {
  const uint32_t W = c->nom_w, R = (uint32_t)gone.size(), cur = c->nom_cur, other = cur ^ 1u;
  if (!R) return BS_OK;
  if (R > W) { c->last_error = "nominated-pod table: more consumed rows than rows"; return BS_ERR_HIP; }
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (nothing of an earlier call still reads the twin)
  HIPCHK(c, nom_reserve(c, other, W - R));
  NomDev a{};
  a.src = nom_tab(c, cur);
  a.dst = nom_tab(c, other);
  a.W = W; a.W2 = W - R; a.N = c->N;
  a.flag = const_cast<uint8_t*>(flag);                      // (k_nm_move reads it; no k_nm_mark: n_remove is 0)
  launch_nom_apply(c->stream, c->S, a, pods_dev(c));
  HIPCHK(c, launch_nom_chains(c, other, W - R));
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<uint32_t> left;
  left.reserve(W - R);
  std::set_difference(c->nom_live.begin(), c->nom_live.end(), gone.begin(), gone.end(), std::back_inserter(left));
  c->nom_live.swap(left);
  c->nom_cur = other;
  c->nom_w = W - R;
  return BS_OK;
}

extern "C" {
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

// The table follows the node list: the host replays the deltas on the node count the table was made for (bs_nominated_nodes_check.hpp over
// bs_bound_nodes_replay.hpp: O(count)) and hands the device the sorted removed OLD nodes; one pass into the twin, which nom_reserve lays
// out for the node count the context holds now, drops the rows on them and renumbers the rest; the chains are made for the new count.
// A list that only grew takes the same path with an empty removed list: nhead's length belongs to the layout.  Two waits: the survivors'
// count sizes the chains' launch, then the dropped rows come back.
int bs_nominated_nodes_apply(bs_ctx* c, uint32_t count, const uint32_t* kind, const uint32_t* index, uint32_t cap, uint32_t* id, uint32_t* node,
                             int32_t* priority, uint32_t* n_out) {
  if (!c) return BS_ERR_INVALID;
  if (nom_nodes_null(count, kind, index, cap, id, node, priority, n_out)) {
    c->last_error = std::string("bs_nominated_nodes_apply: ") + nom_nodes_check_text(kNomNodesNull);
    return BS_ERR_INVALID;
  }
  int rc = nom_single_rank(c, "bs_nominated_nodes_apply");
  if (rc) return rc;
  if (!c->have_nom) { c->last_error = "bs_nominated_nodes_apply: no nominated-pod table (bs_nominated_load first; m = 0 gives the empty one)"; return BS_ERR_STATE; }
  if (!c->have_nodes) { c->last_error = "bs_nominated_nodes_apply: nodes are not loaded"; return BS_ERR_STATE; }
  NodeReplay rp;
  if (const int bad = nom_nodes_check(c->nom_n, c->N, count, kind, index, cap, id, node, priority, n_out, rp)) {
    c->last_error = std::string("bs_nominated_nodes_apply: ") + nom_nodes_check_text(bad);
    return nom_nodes_check_is_state(bad) ? BS_ERR_STATE : BS_ERR_INVALID;
  }
  const uint32_t W = c->nom_w, R = (uint32_t)rp.removed.size();
  *n_out = 0;
  if (!nom_nodes_moves(W, c->nom_n, rp)) {                  // no row, or no old node left and the count kept: nothing is launched
    c->nom_n = rp.n_new;
    return BS_OK;
  }
  if ((rc = use_device(c))) return rc;
  const uint32_t cur = c->nom_cur, other = cur ^ 1u;
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (nothing of an earlier call still reads the twin)
  HIPCHK(c, nom_reserve(c, other, W));
  Carve cv;
  const auto o_rem = cv.take<uint32_t>(R, 4);               // (the call's one H2D block)
  const auto o_info = cv.take<uint32_t>(2);
  const auto o_id = cv.take<uint32_t>(W);
  const auto o_node = cv.take<uint32_t>(W);
  const auto o_prio = cv.take<int32_t>(W);
  if (cv.mark() > c->d_pre.cap) HIPCHK(c, c->d_pre.reserve(cv.mark() + cv.mark() / 4));
  uint8_t* base = c->d_pre.as<uint8_t>();
  if (R) HIPCHK(c, hipMemcpyAsync(o_rem.in(base), rp.removed.data(), o_rem.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(o_info.in(base), 0, o_info.bytes(), c->stream));
  NomNodesDev a{};
  a.src = nom_tab(c, cur);
  a.dst = nom_tab(c, other);
  a.W = W;
  a.rem = o_rem.in(base);
  a.R = R;
  a.o_id = o_id.in(base);
  a.o_node = o_node.in(base);
  a.o_prio = o_prio.in(base);
  a.info = o_info.in(base);
  // Everything above wrote this call's scratch only (and laid the twin out); the live table is read, never written.
  launch_nom_nodes(c->stream, c->S, a);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  uint32_t info[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(info, a.info, sizeof info, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (rp.removed and info are local buffers)
  const uint32_t kept = info[0], left = info[1];
  if (kept + left != W || kept > c->nom_cap[other]) { c->last_error = "bs_nominated_nodes_apply: the counts do not add up to the table"; return BS_ERR_HIP; }
  HIPCHK(c, launch_nom_chains(c, other, kept));
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  std::vector<uint32_t> gone(left);                         // every dropped id: the host's list of live ids follows
  const uint32_t k = std::min(left, cap);
  if (left) HIPCHK(c, hipMemcpyAsync(gone.data(), a.o_id, (size_t)left * 4, hipMemcpyDeviceToHost, c->stream));
  if (k) {
    HIPCHK(c, hipMemcpyAsync(node, a.o_node, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(priority, a.o_prio, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (k) std::memcpy(id, gone.data(), (size_t)k * 4);
  nom_nodes_live_drop(c->nom_live, gone.data(), gone.size());
  c->nom_cur = other;
  c->nom_w = kept;
  c->nom_n = rp.n_new;
  *n_out = left;
  return BS_OK;
}
}  // extern "C"
