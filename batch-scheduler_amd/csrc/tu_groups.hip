// tu_groups.hip — translation unit of group-list surgery (bs_groups_list.hpp: k_gl_gather once per scalar-lane count 0..BS_MAX_SCALARS,
// k_gl_remap), its file-local launch wrappers and the entry points bs_groups_list_apply[_flat] (include/bsched.h).  A unit of its own for
// tu_wait.hip's reason: code added to a unit has changed k_seq_pass's instructions before.
// A family unit: it emits none of the shared headers' non-template kernels (BS_TU_FAMILY, bs_common.hpp).
#ifndef BS_UNITY
#define BS_TU_FAMILY
#endif
#include <cstring>

#include "bs_groups_list.hpp"
#include "bs_groups_list_check.hpp"
#include "bs_ctx.hpp"

namespace bs {

// the columns of a pack laid out by group_carve (bs_layouts.hpp) for `g` groups at `base`
static GlPack gl_pack(const GroupLayout& l, void* base, uint32_t g) {
  GlPack k{};
  group_cols(k, l, base);
  k.stride = std::max<uint32_t>(g, 1);
  return k;
}

// the one pass over the group pack: the map, and every row of the new pack
static void launch_gl_gather(hipStream_t stream, uint32_t S, const GlDev& a) {
  lanes_wide(S, [&](auto s) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gl_gather<decltype(s)::value>), dim3(cdiv(a.g_old + a.n_append, 256)), dim3(256), 0, stream, a);
  });
}
// one group column follows the map; `missing` counts the entries whose group left
static void launch_gl_remap(hipStream_t stream, int32_t* col, uint32_t n, const int32_t* map, uint32_t g_old, uint32_t* missing) {
  if (n) hipLaunchKernelGGL(k_gl_remap, dim3(cdiv(n, 256)), dim3(256), 0, stream, col, n, map, g_old, missing);
}

}  // namespace bs

extern "C" {

// PodGroups enter and leave the cache: the group pack is gathered into its twin, the three tables that hold group indices follow the map.
int bs_groups_list_apply(bs_ctx* c, const bs_groups_list_delta* d, bs_groups_list_out* out) {
  if (!c || !d || !out) return BS_ERR_INVALID;
  if (c->nranks > 1 || c->reduce_external) { c->last_error = "bs_groups_list_apply is single-rank only (as bs_seq_run)"; return BS_ERR_STATE; }
  if (!c->have_groups) { c->last_error = "bs_groups_list_apply before bs_groups_load"; return BS_ERR_STATE; }
  const bs_groups_soa& r = d->rows;
  const bool rows_null = !r.min_member || !r.status_scheduled || !r.matched || !r.flags || !r.cls || !r.min_resources || !r.min_resources_present || !r.occupied_by;
  const bool wait_null = !out->wait_id || !out->wait_node || !out->wait_group;
  const uint32_t g_old = c->G, R = d->n_remove, U = d->n_update, A = d->n_append, L = c->L;
  if (const int bad = groups_list_check(g_old, R, d->remove, U, d->update, r.g, rows_null, A, out->wait_cap, wait_null)) {
    c->last_error = std::string("bs_groups_list_apply: ") + groups_list_text(bad);
    return BS_ERR_INVALID;
  }
  if ((uint64_t)g_old - R + A > 0x7FFFFFFFull) { c->last_error = "bs_groups_list_apply: more groups than a group index can name"; return BS_ERR_CAPACITY; }
  const uint32_t g_new = groups_list_count(g_old, R, A);
  if (!R && !U && !A) {                                     // an empty delta: nothing changes, nothing is launched
    out->g_new = g_old;
    out->n_pods_missing = out->n_bound_missing = out->n_wait_dropped = 0;
    return BS_OK;
  }
  // ---- everything is valid: from here on the resident state changes
  int rc = begin_reload(c);                                 // (a deferred bs_groups_apply patch goes out first, onto the old pack)
  if (rc) return rc;
  c->seq_wait_valid = false;                                // group indices are renumbered
  c->first_reach_hint = 0xFFFFFFFFu;
  // ---- the wait table's rows of removed groups leave by the removal core's release form, while the context still holds the old count
  const bool wait_follows = c->have_wait && c->wait_g == g_old;
  uint32_t n_dropped = 0;
  if (wait_follows && R && c->wait_w &&
      (rc = wait_release_rows(c, "bs_groups_list_apply", R, d->remove, out->wait_cap, out->wait_id, out->wait_node, out->wait_group, &n_dropped)))
    return rc;
  // ---- the delta in pinned memory: its rows as a group pack, then the two lists
  const uint32_t n_rows = U + A;
  Carve bv;
  const GroupLayout rl = group_carve(bv, n_rows, L);
  const auto o_rem = bv.take<uint32_t>(R);
  const auto o_upd = bv.take<uint32_t>(U);
  HIPCHK(c, c->h_glstage.reserve(std::max<size_t>(bv.mark(), 256), std::max<size_t>(bv.mark() + bv.mark() / 4, 4096)));
  uint8_t* st = c->h_glstage.p;
  stage_group_rows(rl, st, r);
  if (R) std::memcpy(o_rem.in(st), d->remove, o_rem.bytes());
  if (U) std::memcpy(o_upd.in(st), d->update, o_upd.bytes());
  // ---- scratch: the map and the three count words
  Carve cv;
  const auto o_cnt = cv.take<uint32_t>(4);
  const auto o_map = cv.take<int32_t>(std::max<uint32_t>(g_old, 1));
  if (cv.mark() > c->d_glist.cap) HIPCHK(c, c->d_glist.reserve(cv.mark() + cv.mark() / 4));
  uint32_t* cnt = o_cnt.in(c->d_glist.p);
  int32_t* map = o_map.in(c->d_glist.p);
  HIPCHK(c, hipMemsetAsync(cnt, 0, o_cnt.bytes(), c->stream));
  // ---- the new pack: the old one under the old layout, the twin under the new one (a quarter of headroom, as the bound and wait tables have)
  GlDev a{};
  a.src = gl_pack(c->glay, c->d_gpack.p, c->G);
  a.g_old = g_old;
  if ((rc = group_layout(c, g_new, true))) return rc;       // the context's layout, count and per-group scratch are now those of g_new
  if (c->glay.bytes > c->d_gpack2.cap) HIPCHK(c, c->d_gpack2.reserve(c->glay.bytes + c->glay.bytes / 4));
  a.dst = gl_pack(c->glay, c->d_gpack2.p, c->G);
  a.rows = gl_pack(rl, st, n_rows);
  a.g_new = g_new;
  a.rem = o_rem.in(st);
  a.upd = o_upd.in(st);
  a.n_remove = R;
  a.n_update = U;
  a.n_append = A;
  a.map = map;
  launch_gl_gather(c->stream, c->S, a);
  LAUNCHCHK(c, BS_KERNEL_PREPASS);
  HIPCHK(c, c->h_glstage.mark_busy(c->stream));
  std::swap(c->d_gpack.p, c->d_gpack2.p);
  std::swap(c->d_gpack.cap, c->d_gpack2.cap);
  // ---- the three group columns follow the map (an identity without a remove: nothing to do)
  if (R) {
    c->pairs_ready = false;                                 // classes stay; pairs, directories, per-group minima and pod ranges are derived again
    c->dirs_ready = false;                                  // from the resident queue by the paths a changed group count already takes
    c->ranges_valid = false;
    if (c->have_pods && c->P) launch_gl_remap(c->stream, c->lay[c->cur_pack].group.in(c->d_pack[c->cur_pack].p), c->P, map, g_old, cnt + 0);
    if (c->have_bound && c->bound_b) launch_gl_remap(c->stream, bound_group_column(c), c->bound_b, map, g_old, cnt + 1);
    if (wait_follows && c->wait_w) launch_gl_remap(c->stream, wait_group_column(c), c->wait_w, map, g_old, cnt + 2);
    LAUNCHCHK(c, BS_KERNEL_PREPASS);
    if (c->have_bound) c->bound_max_group = groups_list_max_group(c->bound_max_group, g_old, R, d->remove);
    if (c->sop_leader0 >= 0 && (uint32_t)c->sop_leader0 < g_old) c->sop_leader0 = groups_list_new_index((uint32_t)c->sop_leader0, R, d->remove);
  }
  if (wait_follows) c->wait_g = g_new;
  uint32_t counts[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(counts, cnt, o_cnt.bytes(), hipMemcpyDeviceToHost, c->stream));
  // ---- what bs_groups_load derives for a new list: the host's view of the flags (the sync), findMaxPG, the positional analysis
  if ((rc = group_counts(c))) return rc;
  if (!g_new) HIPCHK(c, hipStreamSynchronize(c->stream));
  if (counts[2]) { c->last_error = "bs_groups_list_apply: a row of a removed group was still in the wait table"; return BS_ERR_HIP; }
  out->g_new = g_new;
  out->n_pods_missing = counts[0];
  out->n_bound_missing = counts[1];
  out->n_wait_dropped = n_dropped;
  if ((rc = analyse_groups(c))) return rc;
  if ((rc = maybe_analyse_epochs(c))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return BS_OK;
}

int bs_groups_list_apply_flat(bs_ctx* c, uint32_t n_remove, const uint32_t* remove, uint32_t n_update, const uint32_t* update, uint32_t rows_g,
                              const uint32_t* min_member, const uint32_t* status_scheduled, const uint32_t* matched, const uint8_t* flags,
                              const uint32_t* cls, const int64_t* min_resources, const uint32_t* min_resources_present, const uint64_t* occupied_by, uint32_t n_append, uint32_t wait_cap, uint32_t* wait_id,
                              uint32_t* wait_node, int32_t* wait_group, uint32_t* counts_out) {
  if (!counts_out) return BS_ERR_INVALID;
  bs_groups_list_delta d{};
  d.n_remove = n_remove;
  d.remove = remove;
  d.n_update = n_update;
  d.update = update;
  // (bs_groups_soa is shared with bs_groups_read, hence its non-const fields: the call only reads the rows)
  d.rows = bs_groups_soa{rows_g, const_cast<uint32_t*>(min_member), const_cast<uint32_t*>(status_scheduled), const_cast<uint32_t*>(matched),
                         const_cast<uint8_t*>(flags), const_cast<uint32_t*>(cls), const_cast<int64_t*>(min_resources),
                         const_cast<uint32_t*>(min_resources_present), const_cast<uint64_t*>(occupied_by)};
  d.n_append = n_append;
  bs_groups_list_out o{};
  o.wait_cap = wait_cap;
  o.wait_id = wait_id;
  o.wait_node = wait_node;
  o.wait_group = wait_group;
  const int rc = bs_groups_list_apply(c, &d, &o);
  if (rc == BS_OK) {
    counts_out[0] = o.g_new;
    counts_out[1] = o.n_pods_missing;
    counts_out[2] = o.n_bound_missing;
    counts_out[3] = o.n_wait_dropped;
  }
  return rc;
}

}  // extern "C"
