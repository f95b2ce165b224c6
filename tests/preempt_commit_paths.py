"""Which paths k_pc_resolve (csrc/bs_preempt_commit.hpp) has to take for a scene, established on the oracle: pure numpy on top of
tests/preempt_commit_ref.py (and tests/preempt_pdb_ref.py when PDB bits are given), never the library.  The GPU tests of
tests/test_gpu_preempt_commit_chunks.py assert their preconditions on these counts, so that a bit-exact comparison says something about
the record fallback, the rescan, the rescan list's spill and the n_candidates correction — and a mismatch is located by slot, chunk and path.

  geometry(n, count | tiles, forced)   the Python restatement of csrc/bs_preempt_geom.hpp (held against the compiled header by
                                       tests/test_preempt_geom_cpu.py); scalars or numpy arrays
  classify(sc, plan, chunk_nodes)      for every slot in slot order: all nodes evaluated on the BASE state (what k_pc_scan sees), the
                                       candidates ordered by the pick key (the PDB violation count in front when bits are given), split
                                       by chunk; each chunk's record (its best K = 4 keys) classified against the dirty set = the nodes
                                       the reference plan gave to earlier slots."""
from __future__ import annotations

import numpy as np

import preempt_commit_ref as pc
import preempt_ref as pr

K = 4                      # kPcK: pick keys kept per (slot, chunk) record
PREEMPT_WAVES = 4096       # kPreemptWaves
GRID_Y_MAX = 65535         # kPreemptGridYMax
SLOTS_PER_TILE = 64


def cdiv(a, b):
    return (a + b - 1) // b


def geometry(n, count=None, forced=0, tiles=None, waves=PREEMPT_WAVES):
    """(tiles, nchunks, chunk_nodes) as bs::preempt_geom computes them; n / tiles / forced may be numpy arrays (broadcast)"""
    if tiles is None:
        tiles = cdiv(np.asarray(count, np.int64), SLOTS_PER_TILE)
    n, tiles, forced = np.broadcast_arrays(np.asarray(n, np.int64), np.asarray(tiles, np.int64), np.asarray(forced, np.int64))
    n1 = np.maximum(n, 1)
    nch = np.maximum(1, np.minimum(n1, cdiv(waves, tiles)))
    cn = np.maximum(1, cdiv(n, nch))
    nch = np.maximum(1, cdiv(n, cn))
    fcn = np.clip(forced, 1, n1)
    fnch = np.maximum(1, cdiv(n, fcn))
    use = (forced > 0) & (fnch <= GRID_Y_MAX)
    nch, cn = np.where(use, fnch, nch), np.where(use, fcn, cn)
    if nch.ndim == 0:
        return int(tiles), int(nch), int(cn)
    return tiles, nch, cn


def key_order(prep, cand, victim, viol=None):
    """the candidates' pick keys (pre_better, bs_preempt.hpp): (order best first, victim-free mask, violating-victim counts)"""
    prio, st = prep.prio[cand], prep.start[cand]
    vi = viol[cand] if viol is not None else np.zeros(victim.shape, bool)
    rows = np.arange(cand.size)
    nv = victim.sum(axis=1)
    vf = nv == 0
    vv = victim & vi
    npv = vv.sum(axis=1)
    first = np.where(npv > 0, vv.argmax(axis=1), victim.argmax(axis=1))                 # the first listed victim
    top = np.where(vf, 0, prio[rows, first]) if cand.size else np.zeros(0, np.int64)
    mx = np.where(victim, prio, -(1 << 41)).max(axis=1) if cand.size else np.zeros(0, np.int64)
    est = np.where(victim & (prio == mx[:, None]), st, pr.MAX_INT64).min(axis=1) if cand.size else np.zeros(0, np.int64)
    est = np.where(vf, 0, est)
    ssum = np.where(victim, prio + (pr.MAX_INT32 + 1), 0).sum(axis=1)
    return np.lexsort((cand, ~est, nv, ssum, top, npv, ~vf)), vf, npv


def classify(sc: dict, plan: dict, chunk_nodes: int, bits=None, detail: bool = False) -> dict:
    """sc: a scene (preempt_scenes.random_scene's dict); plan: the reference's result dict for it (commit_np / commit_pdb_np's "res");
    chunk_nodes: the geometry under test; bits: the PDB bits the plan was computed with (None: none set).
    Counts are over (slot, chunk) pairs with at least one candidate on the base state:
      entry0       the record's best entry is clean
      later        a later entry is the first clean one (depth[d]: how many at entry d = 1..3)
      rescans      every recorded entry is dirty and the chunk had more than K candidates
      exhausted    every recorded entry is dirty, at most K candidates: the dirty list alone answers for the chunk
      rescans_max / rescans_hist   rescans in one slot: the maximum, and {rescans: slots}
      early_exit   records made of K victim-free nodes (k_pc_scan stops evaluating the chunk's later nodes)
      early_exit_before_violating  ... with a later candidate node of the chunk that holds violating pods
      chosen_dirty       slots whose chosen node an earlier slot had chosen
      ncand_corrected    slots whose n_candidates differs from the base-state count
    detail=True adds "slots": per slot (in slot order) dict(preemptor, later=[(chunk, depth)], rescanned=[chunk], exhausted=[chunk])."""
    S = sc["S"]
    if bits is None:
        prep, ev, viol = pc.CommitPrep(sc["nodes"], sc["bound"], S), pc._eval, None
    else:
        import preempt_pdb_ref as pp
        prep, ev = pp.PdbPrep(sc["nodes"], sc["bound"], S, bits), pp._eval
        viol = prep.viol
    N, L = prep.N, prep.L
    fitb = sc["fit"].to_bool() if N else np.zeros((0, 0), bool)
    prot = np.asarray(sc["protected"], bool) if sc["protected"] is not None and len(sc["protected"]) else np.zeros(1, bool)
    node_viol = viol.any(axis=1) if viol is not None else np.zeros(N, bool)
    chunk_nodes = int(min(max(chunk_nodes, 1), max(N, 1)))
    pods, allcols = sc["pods"], np.arange(N)
    dirty = np.zeros(N, bool)
    out = dict(chunk_nodes=chunk_nodes, nchunks=max(1, cdiv(N, chunk_nodes)), entry0=0, later=0, depth=[0] * K, rescans=0, exhausted=0,
               rescans_max=0, rescans_hist={}, early_exit=0, early_exit_before_violating=0, chosen_dirty=0, ncand_corrected=0)
    slots = []
    for i in pc.slot_order(sc["priority"]):
        pi, P = int(sc["pod_index"][i]), int(sc["priority"][i])
        req = pods.req[:L, pi].astype(np.int64)
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        cand, victim = ev(prep, allcols, prep.valid, prep.cur0, req, pres, cls, grp, P, fitb, prot)
        o, vf, _ = key_order(prep, cand, victim, viol)
        ck, cvf = cand[o], vf[o]
        g = np.argsort(ck // chunk_nodes, kind="stable")                 # by chunk, key order kept inside a chunk
        ck, cvf = ck[g], cvf[g]
        chunks, start, inv, cnt = np.unique(ck // chunk_nodes, return_index=True, return_inverse=True, return_counts=True)
        pos = np.arange(ck.size) - start[inv]
        rec = np.full((chunks.size, K), -1, np.int64)
        recvf = np.zeros((chunks.size, K), bool)
        sel = pos < K
        rec[inv[sel], pos[sel]] = ck[sel]
        recvf[inv[sel], pos[sel]] = cvf[sel]
        clean = (rec >= 0) & ~dirty[np.clip(rec, 0, None)]
        has = clean.any(axis=1)
        depth = clean.argmax(axis=1)
        later = has & (depth > 0)
        resc = ~has & (cnt > K)
        exh = ~has & (cnt <= K)
        out["entry0"] += int((has & (depth == 0)).sum())
        out["later"] += int(later.sum())
        for d in range(1, K):
            out["depth"][d] += int((later & (depth == d)).sum())
        nres = int(resc.sum())
        out["rescans"] += nres
        out["exhausted"] += int(exh.sum())
        out["rescans_max"] = max(out["rescans_max"], nres)
        out["rescans_hist"][nres] = out["rescans_hist"].get(nres, 0) + 1
        early = recvf.all(axis=1)                                       # K victim-free nodes: they are the K lowest of the chunk, rec[:, K-1] the last
        out["early_exit"] += int(early.sum())
        if early.any() and node_viol.any():
            behind = early[inv] & (ck > rec[inv, K - 1]) & node_viol[ck]
            out["early_exit_before_violating"] += int(np.unique(inv[behind]).size)
        k = int(plan["node"][i])
        out["chosen_dirty"] += int(k >= 0 and dirty[k])
        out["ncand_corrected"] += int(int(plan["n_candidates"][i]) != cand.size)
        if detail:
            slots.append(dict(preemptor=int(i), later=[(int(c), int(d)) for c, d in zip(chunks[later], depth[later])],
                              rescanned=chunks[resc].tolist(), exhausted=chunks[exh].tolist()))
        if k >= 0:
            dirty[k] = True
    if detail:
        out["slots"] = slots
    return out


def summary(cl: dict) -> str:
    """one line for a test's output"""
    return (f"chunk_nodes={cl['chunk_nodes']} nchunks={cl['nchunks']} entry0={cl['entry0']} later={cl['later']} depth1..3={cl['depth'][1:]} "
            f"rescans={cl['rescans']} (max {cl['rescans_max']} a slot) exhausted={cl['exhausted']} early_exit={cl['early_exit']} "
            f"(before a violating node: {cl['early_exit_before_violating']}) chosen_dirty={cl['chosen_dirty']} ncand_corrected={cl['ncand_corrected']}")
