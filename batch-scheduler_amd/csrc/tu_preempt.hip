// tu_preempt.hip — translation unit of preemption over the bound-pod table.  Kernels: the victim search (bs_preempt.hpp: k_preempt_scan /
// k_preempt_pick), the sequential plans (bs_preempt_commit.hpp: k_pc_*), the gang plans (bs_preempt_commit_gang.hpp: k_gang_resolve) and the
// plans that clear lower-priority nominations (bs_preempt_clear.hpp: k_nc_resolve), one instantiation per scalar-lane count
// 0..BS_MAX_SCALARS.  Host: their file-local launch wrappers, the entry points bs_preempt_run, _commit and
// _commit_gang (include/bsched.h) and the read-backs of what those calls leave in the context.  The bound table's own calls are tu_bound.hip's
// (the columns: bs_bound_cols.hpp; the swap: bound_twin / bound_swap), the nominated-pod table's are tu_nominated.hip's (nom_*, bs_ctx.hpp;
// NomView is bs_preempt.hpp's): this unit includes the kernel header of neither table's own kernels, k_pdb_* and k_nm_*.
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include "bs_preempt.hpp"
#include "bs_preempt_commit.hpp"
#include "bs_preempt_commit_gang.hpp"
#include "bs_preempt_clear.hpp"
#include "bs_preempt_gang_runs.hpp"
#include "bs_preempt_geom.hpp"
#include "bs_nominated_check.hpp"
#include "bs_bound_cols.hpp"
#include "bs_ctx.hpp"

#include <cstring>

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

// BS_PREEMPT_CLEAR_LOWER with rows in the table, either call: k_pc_scan<S> as above, then k_nc_resolve<S> (bs_preempt_commit hands it
// all-zero run columns)
void launch_preempt_commit_clear(hipStream_t stream, uint32_t S, dim3 scan_grid, const NodesDev& nd, const PodsDev& pd, const CommitDev& pe,
                                 const GangDev& gd, const ClearDev& cd) {
  lanes_wide(S, [&](auto s) {
    constexpr int V = decltype(s)::value;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pc_scan<V>), scan_grid, dim3(64), 0, stream, nd, pd, pe);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nc_resolve<V>), dim3(1), dim3(pc_threads<V>()), 0, stream, nd, pd, pe, gd, cd);
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

}  // namespace

extern "C" {
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
  if (count == 0) { c->pre_npv.clear(); c->have_pre_npv = true; c->have_gang = false; c->have_pre_nom = false; c->pre_clr.reset(false); return BS_OK; }
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
  c->pre_clr.reset(false);
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
// copy and the APPLY tail are one code path.  BS_PREEMPT_CLEAR_LOWER (rule C) with rows in the table: k_nc_resolve<S> for either call (the
// gang columns are carved for both then, all zero for bs_preempt_commit), k_nc_list behind it, and the cleared list in the result copy.
static int preempt_commit_call(bs_ctx* c, uint32_t stages, uint32_t count, const uint32_t* pod_index, const int32_t* priority,
                               const uint8_t* group_protected, const uint32_t* gang_need, bool gang, uint32_t flags, uint32_t victim_cap,
                               const bs_preempt_out* out) {
  if (!c || !out) return BS_ERR_INVALID;
  if (stages & ~BS_STAGE_PREFILTER) { c->last_error = "bs_preempt_commit takes BS_STAGE_PREFILTER only (the plugin's Filter takes no part)"; return BS_ERR_INVALID; }
  if (flags & ~(BS_PREEMPT_APPLY | BS_PREEMPT_ASSUME | BS_PREEMPT_NOMINATE | BS_PREEMPT_CLEAR_LOWER)) { c->last_error = "bs_preempt_commit: unknown flags"; return BS_ERR_INVALID; }
  if ((flags & BS_PREEMPT_ASSUME) && !(flags & BS_PREEMPT_APPLY)) { c->last_error = "BS_PREEMPT_ASSUME needs BS_PREEMPT_APPLY"; return BS_ERR_INVALID; }
  if ((flags & BS_PREEMPT_NOMINATE) && !(flags & BS_PREEMPT_APPLY)) { c->last_error = "BS_PREEMPT_NOMINATE needs BS_PREEMPT_APPLY"; return BS_ERR_INVALID; }
  if ((flags & BS_PREEMPT_NOMINATE) && (flags & BS_PREEMPT_ASSUME)) {
    c->last_error = "BS_PREEMPT_NOMINATE with BS_PREEMPT_ASSUME: the nominee would count twice";
    return BS_ERR_INVALID;
  }
  const bool nominate = (flags & BS_PREEMPT_NOMINATE) != 0, clear = (flags & BS_PREEMPT_CLEAR_LOWER) != 0;
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
    c->pre_clr.reset(clear);
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
  // rule C: k_nc_resolve runs only with the flag AND rows in the table (the refusals above have found the table made for this node list)
  const NomView* const nmv = nom_view(c);
  const bool nc = clear && nmv != nullptr;
  const size_t nW = nc ? std::max<uint32_t>(c->nom_w, 1) : 0;   // (k_nc_list's columns: no bytes in today's blobs)
  Carve cv;
  const auto o_spod = cv.take<uint32_t>(nQ);
  const auto o_sprio = cv.take<int32_t>(nQ);
  const auto o_sorig = cv.take<uint32_t>(nQ);
  const auto o_gprot = cv.take<uint8_t>(nG);
  const size_t gQ = (gang || nc) ? nQ : 0, gB = (gang || nc) ? nB : 0;   // gang columns: no bytes in bs_preempt_commit's blob (k_nc_resolve reads them)
  const size_t cQ = nc ? nQ : 0, cN = nc ? nN : 0;        // rule C's working state
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
  const auto o_cthr = cv.take<uint32_t>(cN);
  const auto o_cfirst = cv.take<uint32_t>(cN);
  const size_t work_bytes = cv.mark() - o_work;
  const auto o_gslog = cv.take<uint32_t>(gQ * 3);
  const auto o_clog = cv.take<uint32_t>(cQ * 2);
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
  const auto o_ccount = cv.take<uint32_t>(nc ? 1 : 0);     // rule C: the cleared list rides the result copy
  const auto o_ccols = cv.take<uint32_t>(nW * 4);
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
  pe.nm = nmv;
  const NodesDev nd = nodes_dev(c);
  if (gang || nc) {
    GangDev gd{};
    gd.s_need = o_gneed.in(base);
    gd.s_rlen = o_grlen.in(base);
    gd.tag = o_gtag.in(base);
    gd.slog = o_gslog.in(base);
    gd.o_placed = o_gplaced.in(base);
    gd.o_voided = o_gvoided.in(base);
    if (nc) {
      ClearDev cd{};
      cd.thr = o_cthr.in(base);
      cd.first = o_cfirst.in(base);
      cd.clog = o_clog.in(base);
      launch_preempt_commit_clear(c->stream, c->S, dim3(tiles, nchunks), nd, pods_dev(c), pe, gd, cd);
      nom_clear_list(c, cd.thr, cd.first, pe.sorig, o_ccols.in(base), o_ccount.in(base));
    } else {
      launch_preempt_commit_gang(c->stream, c->S, dim3(tiles, nchunks), nd, pods_dev(c), pe, gd);
    }
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
  // rule C: what k_nc_list wrote, judged against the ids the context keeps before anything acts on it
  ClearedRows cleared;
  cleared.reset(clear);
  if (nc) {
    const uint32_t W = c->nom_w, n_clr = *o_ccount.in(rb);
    const uint32_t* cols = o_ccols.in(rb);
    if (const int bad = clear_list_check(n_clr, cols, cols + nW, cols + 3 * nW, c->nom_live.data(), W, N, count)) {
      c->last_error = std::string("BS_PREEMPT_CLEAR_LOWER: ") + clear_check_text(bad);
      return BS_ERR_HIP;
    }
    cleared.id.assign(cols, cols + n_clr);
    cleared.node.assign(cols + nW, cols + nW + n_clr);
    cleared.priority.assign(reinterpret_cast<const int32_t*>(cols + 2 * nW), reinterpret_cast<const int32_t*>(cols + 2 * nW) + n_clr);
    cleared.by.assign(cols + 3 * nW, cols + 3 * nW + n_clr);
  }
  if (apply) {
    const uint32_t* info = o_info.in(rb);
    const uint32_t ndirty = info[0], nvall = info[1];
    bs_node_request* dreq = o_nreq.in(base);
    CompactDev nw{};
    const uint32_t B2 = B - nvall;
    BoundLayout lay{};
    if (nvall) HIPCHK(c, bound_twin(c, N, B2, false, lay, &nw));   // the compacted table goes to the second buffer, swapped in below
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
      bound_swap(c, lay, B2);
    }
  }
  std::vector<uint32_t> npod, nnode;
  std::vector<int32_t> nprio;
  if (nominate) {
    // every slot that holds a node (gang: not voided, its node is -1 otherwise) is appended to the table, in the caller's order
    const int32_t* rnode = o_node.in(rb);
    c->pre_nom.assign(nQ, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < count; ++i)
      if (rnode[i] >= 0) {
        c->pre_nom[i] = c->nom_ids + (uint32_t)npod.size();
        npod.push_back(pod_index[i]);
        nnode.push_back((uint32_t)rnode[i]);
        nprio.push_back(priority[i]);
      }
  }
  // one table rewrite: the cleared rows leave (APPLY: their ids are dead from here on), the nominees are appended behind the survivors
  const uint32_t n_gone = apply ? (uint32_t)cleared.id.size() : 0u;
  if ((n_gone || !npod.empty()) &&
      (rc = nom_apply_rows(c, n_gone, cleared.id.data(), (uint32_t)npod.size(), npod.data(), nnode.data(), nprio.data())))
    return rc;
  c->have_pre_nom = nominate;
  c->pre_clr = std::move(cleared);
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

int bs_preempt_cleared_read(bs_ctx* c, uint32_t cap, uint32_t* id, uint32_t* node, int32_t* priority, uint32_t* by, uint32_t* n_out) {
  if (!c) return BS_ERR_INVALID;
  if (const int bad = clear_read(c->pre_clr, cap, id, node, priority, by, n_out)) {
    c->last_error = std::string("bs_preempt_cleared_read: ") + clear_check_text(bad);
    return bad == kClrState ? BS_ERR_STATE : BS_ERR_INVALID;
  }
  return BS_OK;
}
}  // extern "C"
