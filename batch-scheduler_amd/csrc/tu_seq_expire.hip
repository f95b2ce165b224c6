// tu_seq_expire.hip — translation unit of the Permit timeout that undoes the pass's waiting gangs (bs_seq_expire.hpp: k_se_*, the two
// lane-templated kernels once per scalar-lane count 0..BS_MAX_SCALARS), its file-local launch wrappers and the entry points bs_seq_expire /
// bs_seq_waiting_read (include/bsched.h).  A unit of its own, not tu_seq.hip: with these kernels in the pass's unit one instantiation of
// k_seq_pass came out with other instructions (profiles/seq_expire_isa_diff.txt).
// A family unit: it emits none of the shared headers' non-template kernels (BS_TU_FAMILY, bs_common.hpp).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_seq_expire.hpp"
#include "bs_seq_expire_list.hpp"
#include "bs_ctx.hpp"

namespace bs {

// k_se_scan1 + k_se_scan2 (counts, row offsets, the kept groups), k_se_walk (the rows), k_se_sum<S> + k_se_nodes<S> (up to rec_cap bs_node_request
// records for k_nodes_assume, counted in a.info[2]), k_se_groups; nothing when the call has no entries
static void launch_seq_expire(hipStream_t stream, uint32_t S, const SeqExpireDev& a, const PodsDev& pd, const NodesDev& nd, bs_node_request* recs, uint32_t rec_cap) {
  if (!a.M) return;
  const uint32_t nblk = (a.M + kSeBlock - 1) / kSeBlock;
  hipLaunchKernelGGL(k_se_scan1, dim3(nblk), dim3(kSeBlock), 0, stream, a);
  hipLaunchKernelGGL(k_se_scan2, dim3(nblk), dim3(kSeBlock), 0, stream, a);
  hipLaunchKernelGGL(k_se_walk, dim3((a.M + 255) / 256), dim3(256), 0, stream, a, (int32_t*)nullptr);
  if (a.P && rec_cap) lanes_wide(S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_se_sum<decltype(s)::value>), dim3((a.P + 255) / 256), dim3(256), 0, stream, a, pd);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_se_nodes<decltype(s)::value>), dim3((rec_cap + 255) / 256), dim3(256), 0, stream, a, nd.req, nd.rpres, nd.stride, recs);
  });
  hipLaunchKernelGGL(k_se_groups, dim3((a.M + 255) / 256), dim3(256), 0, stream, a);
}

// k_se_walk in its bs_seq_waiting_read form (wait_node pre-filled with -1)
static void launch_seq_waiting(hipStream_t stream, const SeqExpireDev& a, int32_t* wait_node) {
  if (a.G) hipLaunchKernelGGL(k_se_walk, dim3((a.G + 255) / 256), dim3(256), 0, stream, a, wait_node);
}

}  // namespace bs

extern "C" {
static int seq_wait_state(bs_ctx* c, const char* who) {
  if (c->nranks > 1 || c->reduce_external) { c->last_error = std::string(who) + " is single-rank only (as bs_seq_run)"; return BS_ERR_STATE; }
  if (!c->seq_wait_valid || !c->have_nodes || !c->have_groups || !c->have_pods) {
    c->last_error = std::string(who) + ": no valid waiting state (needs a successful bs_seq_run with no queue / node-list / group load or renumbering since)";
    return BS_ERR_STATE;
  }
  return BS_OK;
}

static SeqExpireDev seq_expire_dev(bs_ctx* c) {
  SeqExpireDev a{};
  const GroupsDev gr = groups_dev(c);
  a.wait_rec = c->seq_o_wait.in(c->d_seq.p);
  a.head = c->seq_o_head.in(c->d_seq.p);
  a.nwait = c->seq_o_nwait.in(c->d_seq.p);
  a.P = c->P;
  a.G = c->G;
  a.g_matched = const_cast<uint32_t*>(gr.matched);
  a.g_flags = const_cast<uint8_t*>(gr.flags);
  a.N = c->N;
  return a;
}

int bs_seq_expire(bs_ctx* c, uint32_t count, const uint32_t* group, uint32_t flags, bs_seq_expire_out* out) {
  if (!c || !out) return BS_ERR_INVALID;
  if ((out->group_cap && (!out->group || !out->group_pods || !out->group_earlier)) || (out->pod_cap && (!out->pod || !out->node))) {
    c->last_error = "bs_seq_expire: a result array is NULL with a capacity above 0";
    return BS_ERR_INVALID;
  }
  int rc = seq_wait_state(c, "bs_seq_expire");
  if (rc) return rc;
  if (const int bad = seq_expire_list_check(c->G, count, group, flags)) { c->last_error = seq_expire_list_text(bad); return BS_ERR_INVALID; }
  if ((rc = use_device(c))) return rc;
  if ((rc = settle_pending(c))) return rc;
  out->n_groups = out->n_pods = 0;
  const bool all = (flags & BS_SEQ_EXPIRE_ALL) != 0, deny = (flags & BS_SEQ_EXPIRE_DENY) != 0;
  const uint32_t P = c->P, G = c->G, N = c->N, L = c->L;
  const uint32_t M = all ? G : count;
  if (!M) return BS_OK;
  const uint32_t rec_cap = std::min(N, P), nblk = cdiv(M, kSeBlock);
  // ---- the per-node scratch: zero between calls
  Carve nv;
  const size_t nN = std::max<uint32_t>(N, 1);
  const auto o_delta = nv.take<unsigned long long>(nN * L);
  const auto o_nbits = nv.take<uint32_t>(nN);
  const auto o_dirty = nv.take<uint32_t>(nN);
  {
    const void* was = c->d_sexp_nodes.p;
    HIPCHK(c, c->d_sexp_nodes.reserve(nv.mark()));
    if (!c->sexp_clean || was != c->d_sexp_nodes.p || c->sexp_n != N || c->sexp_l != L) {
      HIPCHK(c, hipMemsetAsync(c->d_sexp_nodes.p, 0, nv.mark(), c->stream));
      c->sexp_n = N;
      c->sexp_l = L;
    }
    c->sexp_clean = false;                                   // until this call's k_se_nodes is known to have run
  }
  Carve cv;
  const auto o_info = cv.take<uint32_t>(4);
  const auto o_list = cv.take<uint32_t>(M);
  const auto o_bsum = cv.take<unsigned long long>(nblk);
  const auto o_group = cv.take<uint32_t>(M);
  const auto o_gpods = cv.take<uint32_t>(M);
  const auto o_gearl = cv.take<uint32_t>(M);
  const auto o_off = cv.take<uint32_t>(M);
  const auto o_pod = cv.take<uint32_t>(std::max<uint32_t>(P, 1));
  const auto o_node = cv.take<uint32_t>(std::max<uint32_t>(P, 1));
  const auto o_dlist = cv.take<uint32_t>(std::max<uint32_t>(rec_cap, 1));
  const auto o_rec = cv.take<bs_node_request>(std::max<uint32_t>(rec_cap, 1));
  HIPCHK(c, c->d_sexp.reserve(cv.mark()));
  void* base = c->d_sexp.p;
  void* nb = c->d_sexp_nodes.p;
  SeqExpireDev a = seq_expire_dev(c);
  a.M = M;
  a.deny = deny ? 1u : 0u;
  a.list = all ? nullptr : o_list.in(base);
  a.bsum = o_bsum.in(base);
  a.info = o_info.in(base);
  a.o_group = o_group.in(base);
  a.o_gpods = o_gpods.in(base);
  a.o_gearlier = o_gearl.in(base);
  a.o_off = o_off.in(base);
  a.o_pod = o_pod.in(base);
  a.o_node = o_node.in(base);
  a.dlist = o_dlist.in(base);
  a.delta = o_delta.in(nb);
  a.nbits = o_nbits.in(nb);
  a.dirty = o_dirty.in(nb);
  bs_node_request* recs = o_rec.in(base);
  HIPCHK(c, hipMemsetAsync(o_info.in(base), 0, o_info.bytes(), c->stream));
  if (!all) HIPCHK(c, hipMemcpyAsync(o_list.in(base), group, o_list.bytes(), hipMemcpyHostToDevice, c->stream));
  c->first_reach_hint = 0xFFFFFFFFu;                        // (as bs_groups_apply: deny entries decide which pod reaches findMaxPG first)
  launch_seq_expire(c->stream, c->S, a, pods_dev(c), nodes_dev(c), recs, rec_cap);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  uint32_t info[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(info, o_info.in(base), o_info.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint32_t ng = info[0], np = info[1], nrec = info[2];
  if (ng > M || np > P || nrec > rec_cap) { c->last_error = "bs_seq_expire: the waiting chains name more than the queue holds"; return BS_ERR_HIP; }
  c->sexp_clean = true;
  // ---- the node requests: k_nodes_assume over the records, the host mirror from their copy (as BS_PREEMPT_APPLY and bs_bound_apply_ex)
  std::vector<uint8_t> hr((size_t)nrec * sizeof(bs_node_request));
  std::vector<uint32_t> hg;
  if (nrec) {
    launch_nodes_assume(c, recs, nrec);
    LAUNCHCHK(c, BS_KERNEL_PREPASS);
    HIPCHK(c, hipMemcpyAsync(hr.data(), recs, hr.size(), hipMemcpyDeviceToHost, c->stream));
    c->bitmap_valid = false;
  }
  const uint32_t kg = std::min(ng, out->group_cap), kp = std::min(np, out->pod_cap);
  if (kg) {
    HIPCHK(c, hipMemcpyAsync(out->group, o_group.in(base), (size_t)kg * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out->group_pods, o_gpods.in(base), (size_t)kg * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out->group_earlier, o_gearl.in(base), (size_t)kg * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (kp) {
    HIPCHK(c, hipMemcpyAsync(out->pod, o_pod.in(base), (size_t)kp * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out->node, o_node.in(base), (size_t)kp * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (deny && all && ng) {
    hg.resize(ng);
    HIPCHK(c, hipMemcpyAsync(hg.data(), o_group.in(base), (size_t)ng * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  mirror_node_requests(c, reinterpret_cast<const bs_node_request*>(hr.data()), nrec);
  if (deny) {
    const uint32_t* gl = all ? hg.data() : group;
    for (uint32_t i = 0; i < ng; ++i) c->h_gflags[gl[i]] |= (uint8_t)BS_GROUP_DENIED;
  }
  out->n_groups = ng;
  out->n_pods = np;
  // findMaxPG, the steady table and the epoch analysis follow the group words as after a bs_groups_apply of these values
  if (ng) {
    if ((rc = analyse_groups(c, false))) return rc;
    if ((rc = maybe_analyse_epochs(c))) return rc;
  }
  return BS_OK;
}

int bs_seq_waiting_read(bs_ctx* c, uint32_t p, int32_t* wait_node) {
  if (!c || (p && !wait_node)) return BS_ERR_INVALID;
  int rc = seq_wait_state(c, "bs_seq_waiting_read");
  if (rc) return rc;
  if (p != c->P) { c->last_error = "bs_seq_waiting_read: p differs from the queue length"; return BS_ERR_INVALID; }
  if ((rc = use_device(c))) return rc;
  if (!p) return BS_OK;
  Carve cv;
  const auto o_wn = cv.take<int32_t>(p);
  HIPCHK(c, c->d_sexp.reserve(cv.mark()));
  int32_t* wn = o_wn.in(c->d_sexp.p);
  HIPCHK(c, hipMemsetAsync(wn, 0xFF, o_wn.bytes(), c->stream));
  launch_seq_waiting(c->stream, seq_expire_dev(c), wn);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  HIPCHK(c, hipMemcpyAsync(wait_node, wn, o_wn.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BS_OK;
}

int bs_seq_expire_flat(bs_ctx* c, uint32_t count, const uint32_t* group, uint32_t flags, uint32_t group_cap, uint32_t* group_out, uint32_t* group_pods,
                       uint32_t* group_earlier, uint32_t pod_cap, uint32_t* pod, uint32_t* node, uint32_t* counts_out) {
  if (!counts_out) return BS_ERR_INVALID;
  bs_seq_expire_out o{};
  o.group_cap = group_cap; o.group = group_out; o.group_pods = group_pods; o.group_earlier = group_earlier;
  o.pod_cap = pod_cap; o.pod = pod; o.node = node;
  const int rc = bs_seq_expire(c, count, group, flags, &o);
  counts_out[0] = o.n_groups;
  counts_out[1] = o.n_pods;
  return rc;
}
}  // extern "C"
