// tu_wait.hip — translation unit of the resident Permit-wait table (bs_wait.hpp: k_wt_*, the lane-templated kernels once per scalar-lane
// count 0..BS_MAX_SCALARS), its file-local launch wrappers and the entry points bs_wait_* (include/bsched.h).  A unit of its own for
// tu_seq_expire.hip's reason: code added to a unit has changed k_seq_pass's instructions before.
// A family unit: it emits none of the shared headers' non-template kernels (BS_TU_FAMILY, bs_common.hpp).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_wait.hpp"
#include "bs_wait_list.hpp"
#include "bs_bound_nodes_replay.hpp"
#include "bs_ctx.hpp"

#include <cstring>

namespace bs {

// the table's one allocation for `cap` rows: columns at 256-byte offsets, req lane stride max(cap, 1)
struct WaitLayout {
  Piece<uint32_t> id;
  Piece<int32_t> group;
  Piece<uint32_t> node, pres;
  Piece<int64_t> req;
  size_t bytes = 0;
  uint32_t stride = 1;
};
static WaitLayout wait_layout(uint32_t cap, uint32_t L) {
  const size_t n = std::max<uint32_t>(cap, 1);
  WaitLayout l;
  Carve cv;
  l.id = cv.take<uint32_t>(n);
  l.group = cv.take<int32_t>(n);
  l.node = cv.take<uint32_t>(n);
  l.pres = cv.take<uint32_t>(n);
  l.req = cv.take<int64_t>(n * L);
  l.bytes = cv.mark();
  l.stride = (uint32_t)n;
  return l;
}
static WaitTab wait_tab(const bs_ctx* c, uint32_t which) {
  const WaitLayout l = wait_layout(c->wait_cap[which], c->L);
  void* b = c->d_wait[which].p;
  return WaitTab{l.id.in(b), l.group.in(b), l.node.in(b), l.pres.in(b), l.req.in(b), l.stride};
}
// rows an allocation is made for: a quarter of headroom (as d_bound2)
static uint32_t wait_room(uint32_t rows) { return std::max<uint32_t>(rows + rows / 4, 256); }
// allocation `which` holds at least `rows` rows afterwards; what it held is lost when it grows
static hipError_t wait_reserve(bs_ctx* c, uint32_t which, uint32_t rows) {
  if (c->d_wait[which].p && c->wait_cap[which] >= rows) return hipSuccess;
  const uint32_t cap = wait_room(rows);
  const hipError_t e = c->d_wait[which].reserve(wait_layout(cap, c->L).bytes);
  if (e == hipSuccess) c->wait_cap[which] = cap;
  return e;
}
// a scratch block that is zero between calls: zeroed when it is new, when it was allocated again (DevBuf::reserve grows by free + malloc,
// and the new block may come back at the old address: the capacity tells, the pointer does not), or when the call before did not get to its end
static hipError_t wait_zeroed(bs_ctx* c, DevBuf& b, size_t bytes, bool& clean) {
  const void* was = b.p;
  const size_t cap_was = b.cap;
  hipError_t e = b.reserve(bytes);
  if (e != hipSuccess) return e;
  if (!clean || was != b.p || cap_was != b.cap) e = hipMemsetAsync(b.p, 0, b.cap, c->stream);
  clean = false;                                            // until the call's last kernel is known to have run
  return e;
}

// k_wt_mark, k_wt_scan1 + k_wt_scan2 (positions, counts, the error word), k_wt_move<S> (the twin, the rows, the per-node sums),
// k_wt_nodes<S> (up to rec_cap records for k_nodes_assume, counted in info[kWtDirty]), k_wt_finish
static void launch_wait_remove(hipStream_t stream, uint32_t S, const WaitDev& a, const NodesDev& nd, bs_node_request* recs, uint32_t rec_cap) {
  if (!a.M) return;
  hipLaunchKernelGGL(k_wt_mark, dim3(cdiv(a.M, 256)), dim3(256), 0, stream, a);
  if (a.W) {
    const uint32_t nblk = cdiv(a.W, kWtBlock);
    hipLaunchKernelGGL(k_wt_scan1, dim3(nblk), dim3(kWtBlock), 0, stream, a);
    hipLaunchKernelGGL(k_wt_scan2, dim3(nblk), dim3(kWtBlock), 0, stream, a);
    lanes_wide(S, [&](auto s) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wt_move<decltype(s)::value>), dim3(cdiv(a.W, 256)), dim3(256), 0, stream, a);
      if (a.node_side && rec_cap)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wt_nodes<decltype(s)::value>), dim3(cdiv(rec_cap, 256)), dim3(256), 0, stream, a, nd.req, nd.rpres, nd.stride, recs);
    });
  }
  hipLaunchKernelGGL(k_wt_finish, dim3(cdiv(a.M, 256)), dim3(256), 0, stream, a);
}

// the table follows node-list surgery: k_wn_map (the one search per row), the spread scan in its by-node face, k_wn_move<S>
static void launch_wait_nodes(hipStream_t stream, uint32_t S, const WaitDev& a) {
  const uint32_t nblk = cdiv(a.W, kWtBlock);
  hipLaunchKernelGGL(k_wn_map, dim3(cdiv(a.W, 256)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(k_wt_scan1, dim3(nblk), dim3(kWtBlock), 0, stream, a);
  hipLaunchKernelGGL(k_wt_scan2, dim3(nblk), dim3(kWtBlock), 0, stream, a);
  lanes_wide(S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wn_move<decltype(s)::value>), dim3(cdiv(a.W, 256)), dim3(256), 0, stream, a);
  });
}

// park, first half: the chains as an array, the scan over the queue
static void launch_wait_park_scan(hipStream_t stream, const WaitDev& a) {
  const uint32_t nblk = cdiv(a.P, kWtBlock);
  hipLaunchKernelGGL(k_wt_walk, dim3(cdiv(a.G, 256)), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(k_wt_scan1, dim3(nblk), dim3(kWtBlock), 0, stream, a);
  hipLaunchKernelGGL(k_wt_scan2, dim3(nblk), dim3(kWtBlock), 0, stream, a);
}
// park, second half: the rows into the table's tail, the chains emptied
static void launch_wait_park_gather(hipStream_t stream, uint32_t S, const WaitDev& a, const PodsDev& pd) {
  lanes_wide(S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wt_gather<decltype(s)::value>), dim3(cdiv(a.P, 256)), dim3(256), 0, stream, a, pd);
  });
  hipLaunchKernelGGL(k_wt_chains, dim3(cdiv(a.G, 256)), dim3(256), 0, stream, a);
}

}  // namespace bs

extern "C" {
static int wait_single_rank(bs_ctx* c, const char* who) {
  if (c->nranks > 1 || c->reduce_external) { c->last_error = std::string(who) + " is single-rank only (as bs_seq_run)"; return BS_ERR_STATE; }
  return BS_OK;
}

// the table exists and was created for the node count and the group count the context holds now
static int wait_table_state(bs_ctx* c, const char* who) {
  if (const int rc = wait_single_rank(c, who)) return rc;
  if (!c->have_wait) { c->last_error = std::string(who) + ": no wait table (bs_wait_load first; w = 0 gives the empty one)"; return BS_ERR_STATE; }
  if (!c->have_nodes || !c->have_groups || c->wait_n != c->N || c->wait_g != c->G) {
    c->last_error = std::string(who) + ": the wait table was created for another node count or group count (after node-list surgery: bs_wait_nodes_apply; else bs_wait_load)";
    return BS_ERR_STATE;
  }
  return BS_OK;
}

int bs_wait_load(bs_ctx* c, uint32_t w, const uint32_t* node, const int32_t* group, const int64_t* req, const uint32_t* req_present) {
  if (!c) return BS_ERR_INVALID;
  int rc = wait_single_rank(c, "bs_wait_load");
  if (rc) return rc;
  if (!c->have_nodes || !c->have_groups) { c->last_error = "bs_wait_load: needs bs_nodes_load and bs_groups_load first"; return BS_ERR_STATE; }
  if (w > BS_WAIT_MAX) { c->last_error = "bs_wait_load: more than BS_WAIT_MAX entries"; return BS_ERR_CAPACITY; }
  if (w && (!node || !group || !req || !req_present)) { c->last_error = "bs_wait_load: a column is NULL with w above 0"; return BS_ERR_INVALID; }
  if (const int bad = wait_load_check(c->N, c->G, w, node, group)) { c->last_error = std::string("bs_wait_load: ") + wait_list_text(bad); return BS_ERR_INVALID; }
  if ((rc = use_device(c))) return rc;
  const uint32_t L = c->L, other = c->wait_cur ^ 1u;
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (nothing of an earlier call still reads the twin)
  HIPCHK(c, wait_reserve(c, other, w));
  const WaitLayout l = wait_layout(c->wait_cap[other], L);
  if (w) {
    // the columns as the table stores them: ids 0 .. w - 1, the pods lane 1, a scalar lane without a present bit 0
    std::vector<uint8_t> st(l.bytes);
    uint32_t* h_id = l.id.in((void*)st.data());
    int32_t* h_group = l.group.in((void*)st.data());
    uint32_t* h_node = l.node.in((void*)st.data());
    uint32_t* h_pres = l.pres.in((void*)st.data());
    int64_t* h_req = l.req.in((void*)st.data());
    const uint32_t smask = c->S ? (uint32_t)((1ull << c->S) - 1ull) : 0u;
    for (uint32_t i = 0; i < w; ++i) {
      h_id[i] = i;
      h_group[i] = group[i];
      h_node[i] = node[i];
      h_pres[i] = req_present[i] & smask;
    }
    for (uint32_t j = 0; j < L; ++j)
      for (uint32_t i = 0; i < w; ++i) {
        int64_t v = req[(size_t)j * w + i];
        if (j == 3) v = 1;
        else if (j > 3 && !((h_pres[i] >> (j - 4)) & 1u)) v = 0;
        h_req[(size_t)j * l.stride + i] = v;
      }
    HIPCHK(c, hipMemcpy(c->d_wait[other].p, st.data(), l.bytes, hipMemcpyHostToDevice));
  }
  c->wait_cur = other;
  c->have_wait = true;
  c->wait_w = c->wait_ids = w;
  c->wait_n = c->N;
  c->wait_g = c->G;
  return BS_OK;
}

int bs_wait_count(const bs_ctx* c, uint32_t* w_out) {
  if (!c || !w_out) return BS_ERR_INVALID;
  if (!c->have_wait) return BS_ERR_STATE;
  *w_out = c->wait_w;
  return BS_OK;
}

int bs_wait_ids(const bs_ctx* c, uint32_t* ids_out) {
  if (!c || !ids_out) return BS_ERR_INVALID;
  if (!c->have_wait) return BS_ERR_STATE;
  *ids_out = c->wait_ids;
  return BS_OK;
}

int bs_wait_read(bs_ctx* c, uint32_t* id, uint32_t* node, int32_t* group, int64_t* req, uint32_t* req_present) {
  if (!c) return BS_ERR_INVALID;
  int rc = wait_table_state(c, "bs_wait_read");
  if (rc) return rc;
  const uint32_t W = c->wait_w;
  if (W && (!id || !node || !group || !req || !req_present)) { c->last_error = "bs_wait_read: a column is NULL and the table has entries"; return BS_ERR_INVALID; }
  if ((rc = use_device(c))) return rc;
  if (!W) return BS_OK;
  const WaitTab t = wait_tab(c, c->wait_cur);
  HIPCHK(c, hipMemcpyAsync(id, t.id, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(node, t.node, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(group, t.group, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(req_present, t.pres, (size_t)W * 4, hipMemcpyDeviceToHost, c->stream));
  for (uint32_t j = 0; j < c->L; ++j)
    HIPCHK(c, hipMemcpyAsync(req + (size_t)j * W, t.req + (size_t)j * t.stride, (size_t)W * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BS_OK;
}

int bs_wait_park(bs_ctx* c, uint32_t cap, uint32_t* pod, uint32_t* node, uint32_t* first_id_out, uint32_t* n_out) {
  if (!c || !first_id_out || !n_out) return BS_ERR_INVALID;
  if (cap && (!pod || !node)) { c->last_error = "bs_wait_park: a result array is NULL with a capacity above 0"; return BS_ERR_INVALID; }
  int rc = wait_single_rank(c, "bs_wait_park");
  if (rc) return rc;
  if (!c->seq_wait_valid || !c->have_nodes || !c->have_groups || !c->have_pods) {
    c->last_error = "bs_wait_park: no valid waiting state (needs a successful bs_seq_run with no queue / node-list / group load or renumbering since)";
    return BS_ERR_STATE;
  }
  if ((rc = wait_table_state(c, "bs_wait_park"))) return rc;
  if ((rc = use_device(c))) return rc;
  const uint32_t P = c->P, G = c->G, W = c->wait_w, L = c->L;
  *first_id_out = c->wait_ids;
  *n_out = 0;
  if (!P || !G) return BS_OK;
  Carve cv;
  const auto o_info = cv.take<uint32_t>(4);
  const auto o_bsum = cv.take<unsigned long long>(cdiv(P, kWtBlock));
  const auto o_pos = cv.take<unsigned long long>(P);
  const auto o_wnode = cv.take<int32_t>(P);
  const auto o_pod = cv.take<uint32_t>(P);
  const auto o_node = cv.take<uint32_t>(P);
  HIPCHK(c, c->d_wait_scr.reserve(cv.mark()));
  void* base = c->d_wait_scr.p;
  WaitDev a{};
  a.mode = kWtPark;
  a.W = W;
  a.E = a.P = P;
  a.G = G;
  a.N = c->N;
  a.ids = c->wait_ids;
  a.wait_rec = c->seq_o_wait.in(c->d_seq.p);
  a.head = c->seq_o_head.in(c->d_seq.p);
  a.nwait = c->seq_o_nwait.in(c->d_seq.p);
  a.info = o_info.in(base);
  a.bsum = o_bsum.in(base);
  a.pos = o_pos.in(base);
  a.wnode = o_wnode.in(base);
  a.o_key = o_pod.in(base);
  a.o_node = o_node.in(base);
  HIPCHK(c, hipMemsetAsync(a.info, 0, o_info.bytes(), c->stream));
  HIPCHK(c, hipMemsetAsync(a.wnode, 0xFF, o_wnode.bytes(), c->stream));
  launch_wait_park_scan(c->stream, a);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  uint32_t info[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(info, a.info, o_info.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint32_t n = info[kWtLeft];
  if (n > P || info[kWtKept] + n != P) { c->last_error = "bs_wait_park: the waiting chains name more than the queue holds"; return BS_ERR_HIP; }
  if (!n) return BS_OK;                                     // (every chain is empty already)
  // All or nothing: so far the call has written its own scratch only (info, wnode, pos) and READ the chains and the queue; the table, its
  // counts, the chains, matched and the node requests are written below this line, by the grow, k_wt_gather and k_wt_chains.
  if ((uint64_t)c->wait_ids + n > BS_WAIT_MAX) { c->last_error = "bs_wait_park: the id space would pass BS_WAIT_MAX"; return BS_ERR_CAPACITY; }
  uint32_t cur = c->wait_cur;
  if (!c->d_wait[cur].p || (uint64_t)W + n > c->wait_cap[cur]) {   // grow: into the twin, the rows so far copied column by column
    const uint32_t other = cur ^ 1u;
    if (c->wait_cap[other] < W + n) c->d_wait[other].release(), c->wait_cap[other] = 0;
    HIPCHK(c, wait_reserve(c, other, W + n));
    if (W) {
      const WaitTab s = wait_tab(c, cur), d = wait_tab(c, other);
      HIPCHK(c, hipMemcpyAsync(d.id, s.id, (size_t)W * 4, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(d.group, s.group, (size_t)W * 4, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(d.node, s.node, (size_t)W * 4, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(d.pres, s.pres, (size_t)W * 4, hipMemcpyDeviceToDevice, c->stream));
      for (uint32_t j = 0; j < L; ++j)
        HIPCHK(c, hipMemcpyAsync(d.req + (size_t)j * d.stride, s.req + (size_t)j * s.stride, (size_t)W * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    c->wait_cur = cur = other;
  }
  a.src = wait_tab(c, cur);
  launch_wait_park_gather(c->stream, c->S, a, pods_dev(c));
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  const uint32_t k = std::min(n, cap);
  if (k) {
    HIPCHK(c, hipMemcpyAsync(pod, a.o_key, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(node, a.o_node, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->wait_w = W + n;
  c->wait_ids += n;
  *n_out = n;
  return BS_OK;
}

// the twin a compaction writes into keeps the table's headroom
static int wait_twin(bs_ctx* c) {
  const uint32_t W = c->wait_w, cur = c->wait_cur, other = cur ^ 1u;
  if (c->d_wait[other].p && c->wait_cap[other] >= std::max(W, c->wait_cap[cur])) return BS_OK;
  const uint32_t cap = std::max(wait_room(W), c->wait_cap[cur]);
  c->d_wait[other].release();
  c->wait_cap[other] = 0;
  HIPCHK(c, c->d_wait[other].reserve(wait_layout(cap, c->L).bytes));
  c->wait_cap[other] = cap;
  return BS_OK;
}

// The removal core behind bs_wait_release (by group), bs_wait_expire (by group, node side, group state) and bs_wait_forget (by id, node
// side, matched - 1 per entry).  l_cnt_out / l_out_out: the per-list-position results (entries per group; unknown per group or node per id).
// group_out (bs_groups_list_apply's release): the rows' groups as a third column beside (id, node).
static int wait_remove(bs_ctx* c, const char* who, uint32_t mode, bool node_side, bool expire, bool deny, uint32_t M, const uint32_t* list, uint32_t cap,
                       uint32_t* id_out, uint32_t* node_out, uint32_t* l_cnt_out, uint32_t* l_out_out, uint32_t* n_out, int32_t* group_out = nullptr) {
  int rc;
  if ((rc = use_device(c))) return rc;
  if (node_side && (rc = settle_pending(c))) return rc;
  const uint32_t W = c->wait_w, N = c->N, G = c->G, L = c->L;
  if (mode == kWtById && !W) { c->last_error = std::string(who) + ": an id is not in the table"; return BS_ERR_INVALID; }
  const uint32_t rec_cap = node_side ? std::min(N, W) : 0u, nblk = cdiv(std::max<uint32_t>(W, 1), kWtBlock);
  // ---- the marks and the per-node scratch: zero between calls
  DevBuf& mk = mode == kWtById ? c->d_wait_imark : c->d_wait_gmark;
  bool& mk_clean = mode == kWtById ? c->wait_imark_clean : c->wait_gmark_clean;
  const uint32_t mark_n = mode == kWtById ? c->wait_ids : G;
  HIPCHK(c, wait_zeroed(c, mk, (size_t)(mk.cap / 4 >= mark_n ? mark_n : wait_room(mark_n)) * 4, mk_clean));
  Carve nv;
  const size_t nN = std::max<uint32_t>(N, 1);
  const auto o_delta = nv.take<unsigned long long>(nN * L);
  const auto o_nbits = nv.take<uint32_t>(nN);
  const auto o_dirty = nv.take<uint32_t>(nN);
  if (node_side) HIPCHK(c, wait_zeroed(c, c->d_wait_nodes, nv.mark(), c->wait_nodes_clean));
  Carve cv;
  const auto o_info = cv.take<uint32_t>(4);
  const auto o_list = cv.take<uint32_t>(M);
  const auto o_lcnt = cv.take<uint32_t>(M);
  const auto o_lout = cv.take<uint32_t>(M);
  const auto o_bsum = cv.take<unsigned long long>(nblk);
  const auto o_pos = cv.take<unsigned long long>(std::max<uint32_t>(W, 1));
  const auto o_id = cv.take<uint32_t>(std::max<uint32_t>(W, 1));
  const auto o_node = cv.take<uint32_t>(std::max<uint32_t>(W, 1));
  const auto o_group = cv.take<int32_t>(group_out ? std::max<uint32_t>(W, 1) : 0u);
  const auto o_dlist = cv.take<uint32_t>(std::max<uint32_t>(rec_cap, 1));
  const auto o_rec = cv.take<bs_node_request>(std::max<uint32_t>(rec_cap, 1));
  HIPCHK(c, c->d_wait_scr.reserve(cv.mark()));
  const uint32_t cur = c->wait_cur, other = cur ^ 1u;
  if ((rc = wait_twin(c))) return rc;
  void* base = c->d_wait_scr.p;
  void* nb = c->d_wait_nodes.p;
  const GroupsDev gr = groups_dev(c);
  WaitDev a{};
  a.src = wait_tab(c, cur);
  a.dst = wait_tab(c, other);
  a.W = a.E = W;
  a.mode = mode;
  a.list = o_list.in(base);
  a.M = M;
  a.mark = mk.as<uint32_t>();
  a.mark_n = mark_n;
  a.node_side = node_side ? 1u : 0u;
  a.forget = mode == kWtById ? 1u : 0u;
  a.expire = expire ? 1u : 0u;
  a.deny = deny ? 1u : 0u;
  a.bsum = o_bsum.in(base);
  a.pos = o_pos.in(base);
  a.info = o_info.in(base);
  a.o_key = o_id.in(base);
  a.o_node = o_node.in(base);
  a.o_group = group_out ? o_group.in(base) : nullptr;
  a.l_cnt = o_lcnt.in(base);
  a.l_out = o_lout.in(base);
  a.delta = node_side ? o_delta.in(nb) : nullptr;
  a.nbits = node_side ? o_nbits.in(nb) : nullptr;
  a.dirty = node_side ? o_dirty.in(nb) : nullptr;
  a.dlist = o_dlist.in(base);
  a.N = N;
  a.g_matched = const_cast<uint32_t*>(gr.matched);
  a.g_flags = const_cast<uint8_t*>(gr.flags);
  a.G = G;
  bs_node_request* recs = o_rec.in(base);
  HIPCHK(c, hipMemsetAsync(a.info, 0, o_info.bytes(), c->stream));
  HIPCHK(c, hipMemsetAsync(a.l_cnt, 0, o_lcnt.bytes(), c->stream));
  HIPCHK(c, hipMemsetAsync(a.l_out, 0, o_lout.bytes(), c->stream));
  HIPCHK(c, hipMemcpyAsync(o_list.in(base), list, o_list.bytes(), hipMemcpyHostToDevice, c->stream));
  launch_wait_remove(c->stream, c->S, a, nodes_dev(c), recs, rec_cap);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  uint32_t info[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(info, a.info, o_info.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  mk_clean = true;
  if (node_side) c->wait_nodes_clean = true;
  if (info[kWtErr]) {                                       // found before k_wt_move wrote anything: the table, the nodes and the groups are as before
    c->last_error = std::string(who) + ((info[kWtErr] & kWtErrTwice) ? ": a group or an id is listed twice" : ": an id is not in the table");
    return BS_ERR_INVALID;
  }
  if (expire) c->first_reach_hint = 0xFFFFFFFFu;            // (as bs_groups_apply: deny entries decide which pod reaches findMaxPG first)
  const uint32_t kept = W ? info[kWtKept] : 0u, left = W ? info[kWtLeft] : 0u, nrec = info[kWtDirty];
  if (kept + left != W || nrec > rec_cap) { c->last_error = std::string(who) + ": the scan's totals do not add up to the table"; return BS_ERR_HIP; }
  if (W) {
    c->wait_cur = other;
    c->wait_w = kept;
  }
  // ---- the node requests: k_nodes_assume over the records, the host mirror from their copy (as bs_seq_expire)
  std::vector<uint8_t> hr((size_t)nrec * sizeof(bs_node_request));
  if (nrec) {
    launch_nodes_assume(c, recs, nrec);
    LAUNCHCHK(c, BS_KERNEL_PREPASS);
    HIPCHK(c, hipMemcpyAsync(hr.data(), recs, hr.size(), hipMemcpyDeviceToHost, c->stream));
    c->bitmap_valid = false;
  }
  const uint32_t k = std::min(left, cap);
  if (k) {
    HIPCHK(c, hipMemcpyAsync(id_out, a.o_key, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(node_out, a.o_node, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    if (group_out) HIPCHK(c, hipMemcpyAsync(group_out, a.o_group, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (l_cnt_out) HIPCHK(c, hipMemcpyAsync(l_cnt_out, a.l_cnt, o_lcnt.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (l_out_out) HIPCHK(c, hipMemcpyAsync(l_out_out, a.l_out, o_lout.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  mirror_node_requests(c, reinterpret_cast<const bs_node_request*>(hr.data()), nrec);
  if (expire && deny)
    for (uint32_t i = 0; i < M; ++i) c->h_gflags[list[i]] |= (uint8_t)BS_GROUP_DENIED;
  if (n_out) *n_out = left;
  // findMaxPG, the steady table and the epoch analysis follow the group words as after a bs_groups_apply of these values
  if (expire || mode == kWtById) {
    if ((rc = analyse_groups(c, false))) return rc;
    if ((rc = maybe_analyse_epochs(c))) return rc;
  }
  return BS_OK;
}

int bs_wait_release(bs_ctx* c, uint32_t count, const uint32_t* group, uint32_t cap, uint32_t* id, uint32_t* node, uint32_t* group_entries, uint32_t* n_out) {
  if (!c || !n_out) return BS_ERR_INVALID;
  if ((count && (!group || !group_entries)) || (cap && (!id || !node))) { c->last_error = "bs_wait_release: an array is NULL with a count or capacity above 0"; return BS_ERR_INVALID; }
  int rc = wait_table_state(c, "bs_wait_release");
  if (rc) return rc;
  if (const int bad = wait_list_check(c->G, count, group)) { c->last_error = std::string("bs_wait_release: ") + wait_list_text(bad); return BS_ERR_INVALID; }
  *n_out = 0;
  if (!count) return BS_OK;
  return wait_remove(c, "bs_wait_release", kWtByGroup, false, false, false, count, group, cap, id, node, group_entries, nullptr, n_out);
}

int bs_wait_expire(bs_ctx* c, uint32_t count, const uint32_t* group, uint32_t flags, uint32_t cap, uint32_t* id, uint32_t* node, uint32_t* group_entries,
                   uint32_t* group_unknown, uint32_t* n_out) {
  if (!c || !n_out) return BS_ERR_INVALID;
  if ((count && (!group || !group_entries || !group_unknown)) || (cap && (!id || !node))) {
    c->last_error = "bs_wait_expire: an array is NULL with a count or capacity above 0";
    return BS_ERR_INVALID;
  }
  int rc = wait_table_state(c, "bs_wait_expire");
  if (rc) return rc;
  int bad = wait_flags_check(flags);
  if (!bad) bad = wait_list_check(c->G, count, group);
  if (bad) { c->last_error = std::string("bs_wait_expire: ") + wait_list_text(bad); return BS_ERR_INVALID; }
  *n_out = 0;
  if (!count) return BS_OK;
  return wait_remove(c, "bs_wait_expire", kWtByGroup, true, true, (flags & kWaitExpireDeny) != 0, count, group, cap, id, node, group_entries, group_unknown, n_out);
}

int bs_wait_forget(bs_ctx* c, uint32_t count, const uint32_t* id, uint32_t* node_out) {
  if (!c) return BS_ERR_INVALID;
  if (count && (!id || !node_out)) { c->last_error = "bs_wait_forget: an array is NULL with a count above 0"; return BS_ERR_INVALID; }
  int rc = wait_table_state(c, "bs_wait_forget");
  if (rc) return rc;
  if (const int bad = wait_list_check(c->wait_ids, count, id)) { c->last_error = std::string("bs_wait_forget: ") + wait_list_text(bad); return BS_ERR_INVALID; }
  if (!count) return BS_OK;
  return wait_remove(c, "bs_wait_forget", kWtById, true, false, false, count, id, 0, nullptr, nullptr, nullptr, node_out, nullptr);
}

// The table follows the node list: the host replays the deltas on the node count the table was made for (bs_bound_nodes_replay.hpp, the
// bound table's replay: O(count)) and hands the device the sorted removed OLD nodes; one pass drops the rows on them and renumbers the rest.
int bs_wait_nodes_apply(bs_ctx* c, uint32_t count, const uint32_t* kind, const uint32_t* index, uint32_t cap, uint32_t* id, uint32_t* node, int32_t* group,
                        uint32_t* n_out) {
  if (!c) return BS_ERR_INVALID;
  if (!n_out || (count && (!kind || !index)) || (cap && (!id || !node || !group))) {
    c->last_error = "bs_wait_nodes_apply: n_out is NULL, or an array is NULL with a count or capacity above 0";
    return BS_ERR_INVALID;
  }
  int rc = wait_single_rank(c, "bs_wait_nodes_apply");
  if (rc) return rc;
  if (!c->have_wait) { c->last_error = "bs_wait_nodes_apply: no wait table (bs_wait_load first; w = 0 gives the empty one)"; return BS_ERR_STATE; }
  if (!c->have_nodes || !c->have_groups || c->wait_g != c->G) {
    c->last_error = "bs_wait_nodes_apply: nodes or groups are not loaded, or the wait table was created for another group count";
    return BS_ERR_STATE;
  }
  NodeReplay rp;
  if (bound_nodes_replay(c->wait_n, count, kind, index, rp)) {
    c->last_error = "bs_wait_nodes_apply: a kind outside UPDATE / APPEND / REMOVE, or an index at or beyond the node count at its point of the replay";
    return BS_ERR_INVALID;
  }
  if (rp.n_new != c->N) { c->last_error = "bs_wait_nodes_apply: the replay does not end at the node count: not the list bs_nodes_apply got"; return BS_ERR_STATE; }
  const uint32_t W = c->wait_w, R = (uint32_t)rp.removed.size(), G = c->G;
  *n_out = 0;
  if (!R || !W) {                                           // no old node left, or no row to sit on one: nothing moves
    c->wait_n = rp.n_new;
    return BS_OK;
  }
  if ((rc = use_device(c))) return rc;
  if ((rc = settle_pending(c))) return rc;
  Carve cv;
  const auto o_info = cv.take<uint32_t>(4);
  const auto o_rem = cv.take<uint32_t>(R);
  const auto o_nnode = cv.take<uint32_t>(W);
  const auto o_bsum = cv.take<unsigned long long>(cdiv(W, kWtBlock));
  const auto o_pos = cv.take<unsigned long long>(W);
  const auto o_id = cv.take<uint32_t>(W);
  const auto o_node = cv.take<uint32_t>(W);
  const auto o_group = cv.take<int32_t>(W);
  HIPCHK(c, c->d_wait_scr.reserve(cv.mark()));
  const uint32_t cur = c->wait_cur, other = cur ^ 1u;
  if ((rc = wait_twin(c))) return rc;
  void* base = c->d_wait_scr.p;
  const GroupsDev gr = groups_dev(c);
  WaitDev a{};
  a.src = wait_tab(c, cur);
  a.dst = wait_tab(c, other);
  a.W = a.E = W;
  a.mode = kWtByNode;
  a.rem = o_rem.in(base);
  a.R = R;
  a.nnode = o_nnode.in(base);
  a.bsum = o_bsum.in(base);
  a.pos = o_pos.in(base);
  a.info = o_info.in(base);
  a.o_key = o_id.in(base);
  a.o_node = o_node.in(base);
  a.o_group = o_group.in(base);
  a.N = c->wait_n;
  a.g_matched = const_cast<uint32_t*>(gr.matched);
  a.G = G;
  HIPCHK(c, hipMemsetAsync(a.info, 0, o_info.bytes(), c->stream));
  HIPCHK(c, hipMemcpyAsync(o_rem.in(base), rp.removed.data(), o_rem.bytes(), hipMemcpyHostToDevice, c->stream));
  // Everything above wrote this call's scratch only; the twin, matched and the counts change from here on.
  launch_wait_nodes(c->stream, c->S, a);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  uint32_t info[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(info, a.info, o_info.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));               // (rp.removed and info are local buffers)
  const uint32_t kept = info[kWtKept], left = info[kWtLeft];
  if (kept + left != W) { c->last_error = "bs_wait_nodes_apply: the scan's totals do not add up to the table"; return BS_ERR_HIP; }
  c->wait_cur = other;
  c->wait_w = kept;
  c->wait_n = rp.n_new;
  const uint32_t k = std::min(left, cap);
  if (k) {
    HIPCHK(c, hipMemcpyAsync(id, a.o_key, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(node, a.o_node, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(group, a.o_group, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *n_out = left;
  if (left) {                                               // matched fell: findMaxPG, the steady table and the epoch analysis follow as after bs_groups_apply
    if ((rc = analyse_groups(c, false))) return rc;
    if ((rc = maybe_analyse_epochs(c))) return rc;
  }
  return BS_OK;
}
}  // extern "C"

namespace bs {
int wait_release_rows(bs_ctx* c, const char* who, uint32_t count, const uint32_t* group, uint32_t cap, uint32_t* id_out, uint32_t* node_out, int32_t* group_out,
                      uint32_t* n_out) {
  return wait_remove(c, who, kWtByGroup, false, false, false, count, group, cap, id_out, node_out, nullptr, nullptr, n_out, group_out);
}
int32_t* wait_group_column(const bs_ctx* c) { return wait_tab(c, c->wait_cur).group; }

// ---- the removal core's launch sequence cut in two for bs_bound_bind (bs_ctx.hpp): by id, no node side, no forget, no expire
static WaitDev wait_bind_core(const WaitBind& wb) {
  WaitDev a{};
  std::memcpy(&a, wb.core.data(), sizeof a);
  return a;
}
int wait_bind_state(bs_ctx* c, const char* who) { return wait_table_state(c, who); }
int wait_bind_front(bs_ctx* c, const char* who, uint32_t n_wait, const uint32_t* wait_id, bool walk, WaitBind& wb) {
  int rc;
  const uint32_t W = n_wait ? c->wait_w : 0u, P = walk ? c->P : 0u, G = c->G;
  if (n_wait && !W) { c->last_error = std::string(who) + ": an id is not in the table"; return BS_ERR_INVALID; }
  const uint32_t mark_n = c->wait_ids;
  if (n_wait) HIPCHK(c, wait_zeroed(c, c->d_wait_imark, (size_t)(c->d_wait_imark.cap / 4 >= mark_n ? mark_n : wait_room(mark_n)) * 4, c->wait_imark_clean));
  Carve cv;
  const auto o_info = cv.take<uint32_t>(4);
  const auto o_list = cv.take<uint32_t>(n_wait);
  const auto o_lcnt = cv.take<uint32_t>(n_wait);
  const auto o_lout = cv.take<uint32_t>(n_wait);
  const auto o_bsum = cv.take<unsigned long long>(cdiv(std::max<uint32_t>(W, 1), kWtBlock));
  const auto o_pos = cv.take<unsigned long long>(std::max<uint32_t>(W, 1));
  const auto o_id = cv.take<uint32_t>(std::max<uint32_t>(W, 1));
  const auto o_node = cv.take<uint32_t>(std::max<uint32_t>(W, 1));
  const auto o_wnode = cv.take<int32_t>(std::max<uint32_t>(P, 1));
  if (cv.mark() > c->d_wait_scr.cap) HIPCHK(c, c->d_wait_scr.reserve(cv.mark() + cv.mark() / 4));
  if (n_wait && (rc = wait_twin(c))) return rc;
  void* base = c->d_wait_scr.p;
  WaitDev a{};
  if (n_wait) {
    a.src = wait_tab(c, c->wait_cur);
    a.dst = wait_tab(c, c->wait_cur ^ 1u);
  }
  a.W = a.E = W;
  a.mode = kWtById;
  a.list = o_list.in(base);
  a.M = n_wait;
  a.mark = c->d_wait_imark.as<uint32_t>();
  a.mark_n = n_wait ? mark_n : 0u;
  a.bsum = o_bsum.in(base);
  a.pos = o_pos.in(base);
  a.info = o_info.in(base);
  a.o_key = o_id.in(base);
  a.o_node = o_node.in(base);
  a.l_cnt = o_lcnt.in(base);
  a.l_out = o_lout.in(base);
  a.N = c->N;
  a.G = G;
  a.wnode = o_wnode.in(base);
  a.P = P;
  HIPCHK(c, hipMemsetAsync(a.info, 0, o_info.bytes(), c->stream));
  if (n_wait) {
    HIPCHK(c, hipMemcpyAsync(o_list.in(base), wait_id, o_list.bytes(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_wt_mark, dim3(cdiv(n_wait, 256)), dim3(256), 0, c->stream, a);
    const uint32_t nblk = cdiv(W, kWtBlock);
    hipLaunchKernelGGL(k_wt_scan1, dim3(nblk), dim3(kWtBlock), 0, c->stream, a);
    hipLaunchKernelGGL(k_wt_scan2, dim3(nblk), dim3(kWtBlock), 0, c->stream, a);
  }
  if (walk && P) {
    a.wait_rec = c->seq_o_wait.in(c->d_seq.p);
    a.head = c->seq_o_head.in(c->d_seq.p);
    a.nwait = c->seq_o_nwait.in(c->d_seq.p);
    HIPCHK(c, hipMemsetAsync(a.wnode, 0xFF, o_wnode.bytes(), c->stream));
    if (G) hipLaunchKernelGGL(k_wt_walk, dim3(cdiv(G, 256)), dim3(256), 0, c->stream, a);
  }
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  wb.id = a.src.id; wb.node = a.src.node; wb.pres = a.src.pres; wb.group = a.src.group; wb.req = a.src.req;
  wb.stride = n_wait ? a.src.stride : 1u;
  wb.W = W;
  wb.mark = a.mark;
  wb.mark_n = a.mark_n;
  wb.info = a.info;
  wb.err = a.info + kWtErr;
  wb.wnode = a.wnode;
  wb.n_wait = n_wait;
  wb.core.resize(sizeof a);
  std::memcpy(wb.core.data(), &a, sizeof a);
  return BS_OK;
}
int wait_bind_back(bs_ctx* c, const WaitBind& wb) {
  if (!wb.n_wait) return BS_OK;
  const WaitDev a = wait_bind_core(wb);
  lanes_wide(c->S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_wt_move<decltype(s)::value>), dim3(cdiv(a.W, 256)), dim3(256), 0, c->stream, a);
  });
  hipLaunchKernelGGL(k_wt_finish, dim3(cdiv(a.M, 256)), dim3(256), 0, c->stream, a);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  return BS_OK;
}
void wait_bind_waited(bs_ctx* c, const WaitBind& wb) {
  if (wb.n_wait) c->wait_imark_clean = true;
}
int wait_bind_verdict(bs_ctx* c, const char* who, const WaitBind& wb, const uint32_t info[4]) {
  if (!wb.n_wait) return BS_OK;
  if (info[kWtErr]) {
    c->last_error = std::string(who) + ((info[kWtErr] & kWtErrTwice) ? ": a wait id is listed twice" : ": a wait id is not in the table");
    return BS_ERR_INVALID;
  }
  if (info[kWtKept] + info[kWtLeft] != wb.W || info[kWtLeft] != wb.n_wait) { c->last_error = std::string(who) + ": the scan's totals do not add up to the table"; return BS_ERR_HIP; }
  return BS_OK;
}
void wait_bind_commit(bs_ctx* c, const WaitBind& wb, const uint32_t info[4]) {
  if (!wb.n_wait) return;
  c->wait_cur ^= 1u;
  c->wait_w = info[kWtKept];
}
}  // namespace bs
