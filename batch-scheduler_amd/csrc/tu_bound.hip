// tu_bound.hip — translation unit of the bound-pod table and its PDB column.  Kernels: the table's patch (bs_bound_apply.hpp: k_ba_*) and its
// remap after node-list surgery (bs_bound_nodes.hpp: k_bn_*), one instantiation per scalar-lane count 0..BS_MAX_SCALARS, and the resident
// PodDisruptionBudgets (bs_pdb.hpp: k_pdb_*, no templates: this unit alone includes that header).  Host: their file-local launch wrappers, the
// entry points bs_bound_* (but bs_bound_bind: tu_bind.hip) and bs_pdb_* (include/bsched.h), and what other units reach the table through
// (bs_ctx.hpp): bound_apply_block, bound_group_column, and bound_twin / bound_swap, the one place where the table's two allocations trade places.
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_bound_apply.hpp"
#include "bs_bound_nodes.hpp"
#include "bs_pdb.hpp"
#include "bs_bound_nodes_replay.hpp"
#include "bs_bound_cols.hpp"
#include "bs_ctx.hpp"

#include <cstring>

namespace {

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

}  // namespace

int32_t* bs::bound_group_column(const bs_ctx* c) { return bound_cols(c->d_bound.as<uint8_t>(), c->blay).group; }

// the table's second allocation laid out for b entries on n nodes (bs_ctx.hpp), and named as a compaction target where one is asked for
hipError_t bs::bound_twin(bs_ctx* c, uint32_t n, uint32_t b, bool headroom, BoundLayout& lay, CompactDev* nw) {
  const size_t bytes = bound_layout(c->L, n, b, lay);
  const hipError_t e = c->d_bound2.reserve(headroom && bytes > c->d_bound2.cap ? bytes + bytes / 4 : bytes);
  if (e != hipSuccess || !nw) return e;
  const auto nt = bound_dev(*nw, c->d_bound2.as<uint8_t>(), lay);
  nw->bpres = nt.pres;
  nw->bnviol = nt.nviol;
  nw->bstride = std::max<uint32_t>(b, 1);
  return e;
}

void bs::bound_swap(bs_ctx* c, const BoundLayout& lay, uint32_t b) {
  std::swap(c->d_bound.p, c->d_bound2.p);
  std::swap(c->d_bound.cap, c->d_bound2.cap);
  c->blay = lay;
  c->bound_b = b;
}

// the back half of every patch of the bound table (bs_ctx.hpp): the second allocation, the merge chain over a delta block that is on the
// device, the one wait, the error word, the swap
int bs::bound_apply_block(bs_ctx* c, const char* who, BoundApplyDev& a, int32_t gmax, const BoundBlockHooks* hooks) {
  const uint32_t N = c->N, B = c->bound_b, ids = c->bound_ids, R = a.n_remove, I = a.n_insert;
  const uint32_t B2 = B - R + I;                           // (when the error word stays clear)
  BoundLayout lay{};
  CompactDev nw{};
  HIPCHK(c, bound_twin(c, N, B2, true, lay, &nw));
  const auto bt = bound_dev(a, c->d_bound.as<const uint8_t>(), c->blay);
  a.bpres = bt.pres;
  a.bstride = std::max<uint32_t>(B, 1);
  a.b = B; a.n = N; a.ids = ids;
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
  bound_swap(c, lay, B2);
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

int bs_bound_count(const bs_ctx* c, uint32_t* b_out) {
  if (!c || !b_out) return BS_ERR_INVALID;
  *b_out = c->have_bound ? c->bound_b : 0u;
  return BS_OK;
}

int bs_bound_load_flat(bs_ctx* c, uint32_t b, const uint32_t* node, const int32_t* priority, const int64_t* start_ns, const int32_t* group,
                       const int64_t* req, const uint32_t* req_present) {
  const bs_bound_soa bd{b, node, priority, start_ns, group, req, req_present};
  return bs_bound_load(c, &bd);
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
  HIPCHK(c, bound_twin(c, N1, B, true, lay));
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
  bound_layout(L, N1, pair[0], lay);                       // as k_bn_move laid it out
  bound_swap(c, lay, pair[0]);
  c->bound_n = N1;
  if (n_dropped_out) *n_dropped_out = pair[1];
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
}  // extern "C"
