// tu_bind.hip — translation unit of bs_bound_bind (include/bsched.h): the kernels of bs_bound_bind.hpp (k_bb_*, once per scalar-lane count
// 0..BS_MAX_SCALARS), their file-local launch wrappers and the entry point.  The wait core's launches stay in tu_wait.hip (wait_bind_*), the
// bound table's merge chain and its swap in tu_bound.hip (bound_apply_block): this unit emits no k_wt_* and no k_ba_* kernel.
// A family unit: it emits none of the shared headers' non-template kernels (BS_TU_FAMILY, bs_common.hpp).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_bound_bind.hpp"
#include "bs_bound_bind_check.hpp"
#include "bs_ctx.hpp"

#include <cstring>

namespace {

// k_bb_rows<S> (the unsorted block, the per-node counts, the error word), k_bb_scan1<S> + k_bb_scan2<S> (the segment starts), k_bb_scatter<S>,
// k_bb_rank<S> (one wave per node), k_bb_gather<S> (the sorted block in BoundApplyDev's insert layout)
template <int S>
void launch_bb_s(hipStream_t stream, const BindDev& a, const PodsDev& pd) {
  const uint32_t items = a.W > a.n_pod ? a.W : a.n_pod;
  if (items) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bb_rows<S>), dim3(cdiv(items, 256)), dim3(256), 0, stream, a, pd);
  if (a.N) {
    const uint32_t nblk = cdiv(a.N, kBbBlock);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bb_scan1<S>), dim3(nblk), dim3(kBbBlock), 0, stream, a);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bb_scan2<S>), dim3(nblk), dim3(kBbBlock), 0, stream, a);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bb_scatter<S>), dim3(cdiv(a.n, 256)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bb_rank<S>), dim3(cdiv(a.N, 4)), dim3(256), 0, stream, a);
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bb_gather<S>), dim3(cdiv(a.n, 256)), dim3(256), 0, stream, a);
}
void launch_bb(hipStream_t stream, uint32_t S, const BindDev& a, const PodsDev& pd) {
  lanes_wide(S, [&](auto s) { launch_bb_s<decltype(s)::value>(stream, a, pd); });
}

}  // namespace

extern "C" {
int bs_bound_bind(bs_ctx* c, uint32_t n_wait, const uint32_t* wait_id, uint32_t n_pod, const uint32_t* pod_index, const int32_t* priority,
                  const int64_t* start_ns, const uint8_t* pdb_violating, uint32_t* node_out, uint32_t* first_id_out) {
  static const char who[] = "bs_bound_bind";
  if (!c) return BS_ERR_INVALID;
  if (c->nranks > 1 || c->reduce_external) { c->last_error = "bs_bound_bind is single-rank only (as bs_seq_run)"; return BS_ERR_STATE; }
  if (!c->have_bound) { c->last_error = "bs_bound_bind before bs_bound_load"; return BS_ERR_STATE; }
  if (c->bound_n != c->N) { c->last_error = "the bound table was loaded for another node list: reload it"; return BS_ERR_STATE; }
  int rc, bad;
  if ((bad = bind_args_check(n_wait, wait_id, n_pod, pod_index, priority, start_ns))) { c->last_error = std::string(who) + ": " + bind_check_text(bad); return BS_ERR_INVALID; }
  const uint32_t ids = c->bound_ids;
  if (!n_wait && !n_pod) {
    if (first_id_out) *first_id_out = ids;
    return BS_OK;
  }
  if (n_wait && (rc = wait_bind_state(c, who))) return rc;
  if (n_pod && (!c->seq_wait_valid || !c->have_nodes || !c->have_groups || !c->have_pods)) {
    c->last_error = "bs_bound_bind: no valid pass results (needs a successful bs_seq_run with no queue / node-list / group load or renumbering since)";
    return BS_ERR_STATE;
  }
  if ((bad = bind_lists_check(c->wait_ids, c->wait_w, n_wait, wait_id, c->P, n_pod, pod_index))) { c->last_error = std::string(who) + ": " + bind_check_text(bad); return BS_ERR_INVALID; }
  if ((bad = bind_ids_check(ids, n_wait, n_pod, BS_BOUND_MAX))) { c->last_error = std::string(who) + ": " + bind_check_text(bad); return BS_ERR_CAPACITY; }
  if ((rc = use_device(c))) return rc;
  const uint32_t n = n_wait + n_pod, N = c->N, L = c->L, P = n_pod ? c->P : 0u, B = c->bound_b;
  // ---- the wait core's front half: the marks, the positions, the chains as an array
  WaitBind wb;
  if ((rc = wait_bind_front(c, who, n_wait, wait_id, n_pod != 0, wb))) return rc;
  // ---- one allocation: the host's blob (8-byte column first), the sorted block, the unsorted rows, the patch's scratch and this call's
  const size_t nn = n, nN = std::max<uint32_t>(N, 1);
  Carve cv;
  const auto o_hstart = cv.take<int64_t>(nn, 1);           // (packed)
  const auto o_hprio = cv.take<int32_t>(nn, 1);
  const auto o_plist = cv.take<uint32_t>(n_pod, 1);
  const auto o_hpdb = cv.take<uint8_t>(nn);                // the last column: what follows starts at the next 256
  const size_t blob_bytes = o_hpdb.off + o_hpdb.bytes();
  const auto o_istart = cv.take<int64_t>(nn);
  const auto o_ireq = cv.take<int64_t>(nn * L);
  const auto o_inode = cv.take<uint32_t>(nn);
  const auto o_iprio = cv.take<int32_t>(nn);
  const auto o_igroup = cv.take<int32_t>(nn);
  const auto o_iid = cv.take<uint32_t>(nn);
  const auto o_ipres = cv.take<uint32_t>(nn);
  const auto o_ipdb = cv.take<uint8_t>(nn);
  const auto o_ureq = cv.take<int64_t>(nn * L);
  const auto o_unode = cv.take<uint32_t>(nn);
  const auto o_ugroup = cv.take<int32_t>(nn);
  const auto o_upres = cv.take<uint32_t>(nn);
  const auto o_posof = cv.take<uint32_t>(std::max<uint32_t>(ids, 1));
  const size_t o_zero = cv.mark();
  const auto o_res = cv.take<uint32_t>(4);
  const auto o_deadw = cv.take<uint32_t>((size_t)B / 32 + 1);
  const auto o_dcnt = cv.take<uint32_t>(nN);
  const auto o_icnt = cv.take<uint32_t>(nN);
  const auto o_ncnt = cv.take<uint32_t>(nN);
  const auto o_ncur = cv.take<uint32_t>(nN);
  const auto o_claim = cv.take<uint32_t>((size_t)P / 32 + 1);
  const size_t zero_bytes = cv.mark() - o_zero;
  const auto o_ifirst = cv.take<uint32_t>(nN);
  const auto o_noff = cv.take<uint32_t>(nN + 1);
  const auto o_bsum = cv.take<uint32_t>(cdiv((uint32_t)nN, kBbBlock));
  const auto o_seg = cv.take<uint32_t>(nn);
  const auto o_perm = cv.take<uint32_t>(nn);
  const auto o_nout = cv.take<uint32_t>(nn);
  // the id space grows with every call: a quarter of headroom, so that a run of calls allocates rarely
  if (cv.mark() > c->d_pre.cap) HIPCHK(c, c->d_pre.reserve(cv.mark() + cv.mark() / 4));
  std::vector<uint8_t> h(blob_bytes, 0);
  uint8_t* hb = h.data();
  std::memcpy(o_hstart.in(hb), start_ns, o_hstart.bytes());
  std::memcpy(o_hprio.in(hb), priority, o_hprio.bytes());
  if (n_pod) std::memcpy(o_plist.in(hb), pod_index, o_plist.bytes());
  if (pdb_violating)
    for (uint32_t i = 0; i < n; ++i) o_hpdb.in(hb)[i] = pdb_violating[i] ? 1 : 0;
  uint8_t* base = c->d_pre.as<uint8_t>();
  HIPCHK(c, hipMemcpyAsync(base, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(o_posof.in(base), 0xff, o_posof.bytes(), c->stream));
  HIPCHK(c, hipMemsetAsync(base + o_zero, 0, zero_bytes, c->stream));
  BindDev d{};
  d.w_id = wb.id; d.w_group = wb.group; d.w_node = wb.node; d.w_pres = wb.pres; d.w_req = wb.req;
  d.w_stride = wb.stride;
  d.W = wb.W;
  d.mark = wb.mark;
  d.mark_n = wb.mark_n;
  d.w_err = wb.err;
  d.plist = o_plist.in(base);
  d.pod_node = n_pod ? c->seq_o_node.in(c->d_seq.p) : nullptr;
  d.wnode = wb.wnode;
  d.claim = o_claim.in(base);
  d.n_wait = n_wait; d.n_pod = n_pod; d.n = n;
  d.P = P; d.N = N; d.ids = ids;
  d.u_node = o_unode.in(base); d.u_group = o_ugroup.in(base); d.u_pres = o_upres.in(base); d.u_req = o_ureq.in(base);
  d.h_prio = o_hprio.in(base); d.h_start = o_hstart.in(base); d.h_pdb = o_hpdb.in(base);
  d.ncnt = o_ncnt.in(base); d.ncur = o_ncur.in(base); d.noff = o_noff.in(base); d.bsum = o_bsum.in(base);
  d.seg = o_seg.in(base); d.perm = o_perm.in(base);
  d.res = o_res.in(base);
  d.node_out = o_nout.in(base);
  d.inode = o_inode.in(base); d.iprio = o_iprio.in(base); d.istart = o_istart.in(base); d.igroup = o_igroup.in(base);
  d.ireq = o_ireq.in(base); d.iid = o_iid.in(base); d.ipres = o_ipres.in(base); d.ipdb = o_ipdb.in(base);
  launch_bb(c->stream, c->S, d, pods_dev(c));
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  // ---- the patch over the block the device built, then the wait core's back half; one wait for both
  BoundApplyDev a{};
  a.n_remove = 0; a.n_insert = n;
  a.inode = d.inode; a.iprio = d.iprio; a.istart = d.istart; a.igroup = d.igroup; a.ireq = d.ireq; a.iid = d.iid; a.ipres = d.ipres; a.ipdb = d.ipdb;
  a.pos_of = o_posof.in(base);
  a.deadw = o_deadw.in(base);
  a.dcnt = o_dcnt.in(base);
  a.icnt = o_icnt.in(base);
  a.ifirst = o_ifirst.in(base);
  a.err = d.res + kBbResBa;
  uint32_t res[4] = {0, 0, 0, 0}, info[4] = {0, 0, 0, 0};
  std::vector<uint32_t> nout(n);
  BoundBlockHooks hooks;
  hooks.before_wait = [&]() -> int {
    if (const int r = wait_bind_back(c, wb)) return r;
    HIPCHK(c, hipMemcpyAsync(res, d.res, sizeof res, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(info, wb.info, sizeof info, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nout.data(), d.node_out, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    return BS_OK;
  };
  hooks.verdict = [&](uint32_t ba_err, int32_t& gmax) -> int {
    wait_bind_waited(c, wb);
    if (const int r = wait_bind_verdict(c, who, wb, info)) return r;
    if (const uint32_t e = res[kBbResErr]) {
      c->last_error = std::string(who) + ((e & kBbErrRange)    ? ": a pod index is at or above the queue length"
                                          : (e & kBbErrTwice)  ? ": a pod index is listed twice"
                                          : (e & kBbErrNoNode) ? ": a listed pod has no node from the last pass"
                                          : (e & kBbErrWaits)  ? ": a listed pod still waits at Permit (parked, not bound)"
                                                               : ": a row names a node outside the node list");
      return BS_ERR_INVALID;
    }
    // a segment k_bb_rank left (longer than the limit) leaves the sorted block unwritten, and k_ba_mark may then add kBaErrNode: the limit rules
    if (ba_err & kBaErrFull) { c->last_error = std::string(who) + ": more than BS_BOUND_MAX_PER_NODE bound pods on one node"; return BS_ERR_CAPACITY; }
    if (res[kBbResGroup]) gmax = std::max(gmax, (int32_t)(res[kBbResGroup] - 1u) + BS_POD_GROUP_MISSING);
    return BS_OK;
  };
  if ((rc = bound_apply_block(c, who, a, c->bound_max_group, &hooks))) return rc;
  wait_bind_commit(c, wb, info);
  if (node_out) std::memcpy(node_out, nout.data(), (size_t)n * 4);
  if (first_id_out) *first_id_out = ids;
  return BS_OK;
}
}  // extern "C"
