"""Two independent CPU restatements of PDB-aware preemption (include/bsched.h: bs_bound_pdb_set, steps 5 and 6 of bs_preempt_run, the
library rule of bs_preempt_commit), for the single call and for the sequence, built on tests/preempt_ref.py and
tests/preempt_commit_ref.py by import.

Recalled upstream semantics (k8s v1.17.5 generic_scheduler.go; the source is not vendored, so they are written out once here and once
in the header as D1..D4):
  D1. filterPodsWithPDBViolation is a static test per pod (some PDB of its namespace whose selector matches its labels has
      PodDisruptionsAllowed <= 0); no budget is counted down while victims are chosen.  Here: violating[id] per bound pod.
  D2. selectVictimsOnNode sorts the potential victims by MoreImportantPod, splits them into violatingVictims and nonViolatingVictims
      (each keeps the order), reprieves all of the former first and then the latter, counts numViolatingVictim among the former
      only, and returns the victims in that order.
  D3. pickOneNodeForPreemption: a victim-free node first; then the fewest PDB violations; then the lowest victims.Pods[0] priority
      (the FIRST LISTED victim, not the maximum); then the smallest sum of priority + 2^31, the fewest victims, the latest
      GetEarliestPodStartTime (earliest start among the victims of the true maximum priority); ties to the lowest node index.
  D4. a pod of priority >= the preemptor's is no potential victim; its bit is never looked at.

  preempt_pdb_obj / commit_pdb_obj   object level: pod dicts, the split, the two reprieve loops, the pick as filtering passes.
  preempt_pdb_np / commit_pdb_np     numpy over node columns: what the GPU is held against.

All return what their counterparts in preempt_ref / preempt_commit_ref return, plus n_pdb_violations[count] in the result dict."""
from __future__ import annotations

import functools
import json
import os

import numpy as np

import preempt_commit_ref as pc
import preempt_ref as pr

MAX_INT32 = pr.MAX_INT32
FIELDS = ("node", "n_candidates", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start", "n_pdb_violations")


def _empty(q: int, cap: int) -> dict:
    out = pr._empty(q, cap)
    out["n_pdb_violations"] = np.zeros(q, np.uint32)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# object level
# ------------------------------------------------------------------------------------------------------------------------------
def select_victims_on_node(nodes, k, pods_on_node, q_req, q_pres, q_group, P, protected, S, violating):
    """selectVictimsOnNode with PDBs (D2): (victims in reprieve order, numViolatingVictim, fits)"""
    ni = pr._node_info(nodes, k, S)
    potential = []
    for p in pods_on_node:
        if p["priority"] < P:                               # D4
            potential.append(p)
            pr._remove_pod(ni, p)
            if pr.remove_policy(q_group, p["group"], protected) is not None:
                return None, 0, False
    if not pr.holds_obj(nodes, k, ni, q_req, q_pres, S):
        return None, 0, False
    potential.sort(key=functools.cmp_to_key(pr._more_important))
    violating_victims = [p for p in potential if violating[p["id"]]]
    non_violating_victims = [p for p in potential if not violating[p["id"]]]
    victims, num_violating = [], 0

    def reprieve(p) -> bool:
        pr._add_pod(ni, p)
        fits = pr.holds_obj(nodes, k, ni, q_req, q_pres, S)
        if not fits:
            pr._remove_pod(ni, p)
            victims.append(p)
        return fits

    for p in violating_victims:
        if not reprieve(p):
            num_violating += 1
    for p in non_violating_victims:
        reprieve(p)
    return victims, num_violating, True


def pick_one_node(nodes_to_victims: dict, violations: dict):
    """pickOneNodeForPreemption (D3) over {node: victims} and {node: numPDBViolations}"""
    if not nodes_to_victims:
        return None
    order = sorted(nodes_to_victims)
    for node in order:
        if len(nodes_to_victims[node]) == 0:
            return node
    min_viol, min_nodes = MAX_INT32, []
    for node in order:
        n = violations[node]
        if n < min_viol:
            min_viol, min_nodes = n, [node]
        elif n == min_viol:
            min_nodes.append(node)
    if len(min_nodes) == 1:
        return min_nodes[0]
    # the remaining passes are preempt_ref.pick_one_node's: Pods[0] priority, sum, count, latest GetEarliestPodStartTime
    return pr.pick_one_node({node: nodes_to_victims[node] for node in min_nodes})


def _search_obj(state, fitb, per, req, pres, cls, grp, P, protected, S, violating):
    nv, viol = {}, {}
    for k in range(state.n):
        if state.flags[k] or cls >= fitb.shape[0] or not fitb[cls, k]:
            continue
        victims, nviol, ok = select_victims_on_node(state, k, per.get(k, []), req, pres, grp, P, protected, S, violating)
        if ok:
            nv[k], viol[k] = victims, nviol
    return nv, viol


def _fill(out, i, node, v, nviol, cap):
    out["node"][i] = node
    out["n_victims"][i] = len(v)
    for j, p in enumerate(v[:cap]):
        out["victims"][i, j] = p["id"]
    if v:
        out["top_priority"][i] = v[0]["priority"]           # Pods[0]
        out["priority_sum"][i] = sum(p["priority"] + (MAX_INT32 + 1) for p in v)
        out["earliest_start"][i] = pr.earliest_start(v)
        out["n_pdb_violations"][i] = nviol


def preempt_pdb_obj(nodes, fit, pods, bound, S, pod_index, priority, protected, cap, violating) -> dict:
    per = pr.bound_objects(bound, S)
    fitb = fit.to_bool()
    q = len(pod_index)
    out = _empty(q, cap)
    for i in range(q):
        pi, P = int(pod_index[i]), int(priority[i])
        req = [int(pods.req[j, pi]) for j in range(4 + S)]
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        nv, viol = _search_obj(nodes, fitb, per, req, pres, cls, grp, P, protected, S, violating)
        out["n_candidates"][i] = len(nv)
        node = pick_one_node(nv, viol)
        if node is not None:
            _fill(out, i, node, nv[node], viol[node], cap)
    return out


def commit_pdb_obj(nodes, fit, pods, bound, S, pod_index, priority, protected, cap, violating, apply=False, assume=False) -> dict:
    """preempt_commit_ref.commit_obj with the PDB-aware search; the bits are fixed for the whole call (the library rule)"""
    per = pr.bound_objects(bound, S)
    for k in per:
        per[k].sort(key=functools.cmp_to_key(pr._more_important))
    work, final = pc._NodeState(nodes), pc._NodeState(nodes)
    fitb = fit.to_bool()
    q = len(pod_index)
    out = _empty(q, cap)
    for i in pc.slot_order(priority):
        pi, P = int(pod_index[i]), int(priority[i])
        req = [int(pods.req[j, pi]) for j in range(4 + S)]
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        nv, viol = _search_obj(work, fitb, per, req, pres, cls, grp, P, protected, S, violating)
        out["n_candidates"][i] = len(nv)
        node = pick_one_node(nv, viol)
        if node is None:
            continue
        v = nv[node]
        _fill(out, i, node, v, viol[node], cap)
        gone = {p["id"] for p in v}
        per[node] = [p for p in per.get(node, []) if p["id"] not in gone]
        nom = pc._pod_obj(pods, pi, S)
        for st, add in ((work, True), (final, assume)):
            ni = pr._node_info(st, node, S)
            for p in v:
                pr._remove_pod(ni, p)
            if add:
                pr._add_pod(ni, nom)
            st.put(node, ni)
    if not apply:
        final = pc._NodeState(nodes)
        per = pr.bound_objects(bound, S)
        for k in per:
            per[k].sort(key=functools.cmp_to_key(pr._more_important))
    ids = [p["id"] for k in sorted(per) for p in per[k]]
    nodes_of = [k for k in sorted(per) for _ in per[k]]
    return dict(res=out, req=final.requested, pres=final.requested_present, bound_id=np.array(ids, np.uint32),
                bound_node=np.array(nodes_of, np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------
# numpy
# ------------------------------------------------------------------------------------------------------------------------------
class PdbPrep(pc.CommitPrep):
    """preempt_commit_ref.CommitPrep plus the bit of every table entry, viol [N, M]"""

    def __init__(self, nodes, bound, S: int, violating=None):
        super().__init__(nodes, bound, S)
        self.viol = np.zeros((self.N, self.M), bool)
        if violating is not None and bound.b:
            self.viol[self.valid] = np.asarray(violating).reshape(-1)[self.id[self.valid]] != 0


def _eval(prep, cols, valid, cur, req, pres, cls, grp, P, fitb, prot):
    """steps 1-5 on the node columns `cols`: (candidate nodes, victim mask [c, M]); the reprieve runs the violating entries of every
    node first (all table columns), then the others"""
    S = prep.S
    ok = prep.flags[cols] == 0
    ok &= fitb[cls, cols] if cls < fitb.shape[0] else np.zeros(cols.size, bool)
    g = prep.group[cols]
    vm = valid[cols] & (prep.prio[cols] < P)
    q_grouped = grp != pr.NOT_GROUPED
    v_bad = (g == pr.GROUP_MISSING) | ((g >= 0) & prot[np.clip(g, 0, None)])
    bad = np.where(g == pr.NOT_GROUPED, q_grouped, v_bad | (q_grouped & (g == grp)))
    ok &= ~np.any(vm & bad, axis=1)
    with np.errstate(over="ignore"):
        c = cur[:, cols] - (prep.req[:, cols] * vm[None]).sum(axis=2)
    ok &= pr.holds_np(prep.alloc[:, cols], prep.apres[cols], c, req, pres, S)
    sel = np.nonzero(ok)[0]
    cand, m, c = cols[sel], vm[sel], c[:, sel]
    al, ap, rq, vi = prep.alloc[:, cand], prep.apres[cand], prep.req[:, cand], prep.viol[cand]
    victim = np.zeros(m.shape, bool)
    with np.errstate(over="ignore"):
        for part in (m & vi, m & ~vi):
            for col in range(prep.M):
                mc = part[:, col]
                if not mc.any():
                    continue
                t = c + rq[:, :, col] * mc[None]
                h = pr.holds_np(al, ap, t, req, pres, S)
                c = np.where((mc & h)[None], t, c)
                victim[:, col] |= mc & ~h
    return cand, victim


def _pick(prep, cand, victim, out, i, cap):
    """step 6 over the candidates (ascending node index); fills row i and returns (node, victim mask of it) or (None, None)"""
    out["n_candidates"][i] = cand.size
    if cand.size == 0:
        return None, None
    prio, st, vi = prep.prio[cand], prep.start[cand], prep.viol[cand]
    nv = victim.sum(axis=1)
    rows = np.arange(cand.size)
    if np.any(nv == 0):
        w = int(np.nonzero(nv == 0)[0][0])
    else:
        vv = victim & vi
        npv = vv.sum(axis=1)
        first = np.where(npv > 0, vv.argmax(axis=1), victim.argmax(axis=1))      # the first listed victim
        top = prio[rows, first]
        mx = np.where(victim, prio, -(1 << 40)).max(axis=1)
        est = np.where(victim & (prio == mx[:, None]), st, pr.MAX_INT64).min(axis=1)
        ssum = np.where(victim, prio + (MAX_INT32 + 1), 0).sum(axis=1)
        w = int(np.lexsort((cand, ~est, nv, ssum, top, npv))[0])
        out["top_priority"][i] = top[w]
        out["priority_sum"][i] = ssum[w]
        out["earliest_start"][i] = est[w]
        out["n_pdb_violations"][i] = npv[w]
    k = int(cand[w])
    out["node"][i] = k
    out["n_victims"][i] = nv[w]
    vm = victim[w]
    vid = np.concatenate([prep.id[k][vm & prep.viol[k]], prep.id[k][vm & ~prep.viol[k]]])
    out["victims"][i, : min(vid.size, cap)] = vid[:cap]
    return k, vm


def _common(prep, fit, protected):
    fitb = fit.to_bool() if prep.N else np.zeros((0, 0), bool)
    prot = np.asarray(protected, bool) if protected is not None and len(protected) else np.zeros(1, bool)
    return fitb, prot


def preempt_pdb_np(prep: PdbPrep, fit, pods, pod_index, priority, protected, cap) -> dict:
    fitb, prot = _common(prep, fit, protected)
    q = len(pod_index)
    out = _empty(q, cap)
    allcols = np.arange(prep.N)
    for i in range(q):
        pi, P = int(pod_index[i]), int(priority[i])
        req = pods.req[: prep.L, pi].astype(np.int64)
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        cand, victim = _eval(prep, allcols, prep.valid, prep.cur0, req, pres, cls, grp, P, fitb, prot)
        _pick(prep, cand, victim, out, i, cap)
    return out


def commit_pdb_np(prep: PdbPrep, fit, pods, bound, pod_index, priority, protected, cap, apply=False, assume=False) -> dict:
    """preempt_commit_ref.commit_np with the PDB-aware search and pick"""
    S, L, N = prep.S, prep.L, prep.N
    fitb, prot = _common(prep, fit, protected)
    alive = prep.valid.copy()
    cur = prep.cur0.copy()
    dv, dn = np.zeros((L, N), np.int64), np.zeros((L, N), np.int64)
    vbits, nbits = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    touched = np.zeros(N, bool)
    bpres = np.zeros((N, prep.M), np.uint32)
    bpres[prep.valid] = bound.req_present[prep.id[prep.valid]]
    smask = np.uint32((1 << S) - 1)
    q = len(pod_index)
    out = _empty(q, cap)
    allcols = np.arange(N)
    for i in pc.slot_order(priority):
        pi, P = int(pod_index[i]), int(priority[i])
        req = pods.req[:L, pi].astype(np.int64)
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        c1, v1 = _eval(prep, allcols[~touched], prep.valid, prep.cur0, req, pres, cls, grp, P, fitb, prot)
        c2, v2 = _eval(prep, allcols[touched], alive, cur, req, pres, cls, grp, P, fitb, prot)
        cand, victim = np.concatenate([c1, c2]), np.concatenate([v1, v2])
        o = np.argsort(cand, kind="stable")
        k, vm = _pick(prep, cand[o], victim[o], out, i, cap)
        if k is None:
            continue
        nom = req.copy()
        nom[3] = 1
        for s in range(S):
            if not (pres >> s) & 1:
                nom[4 + s] = 0
        with np.errstate(over="ignore"):
            gone = prep.req[:, k][:, vm].sum(axis=1)
            cur[:, k] = cur[:, k] - gone + nom
            dv[:, k] += gone
            dn[:, k] += nom
        alive[k] &= ~vm
        vbits[k] |= np.bitwise_or.reduce(bpres[k][vm]) if vm.any() else np.uint32(0)
        nbits[k] |= np.uint32(pres) & smask
        touched[k] = True
    raw, rp = prep.raw_req.copy(), prep.raw_pres.copy()
    if apply:
        for k in np.nonzero(touched)[0]:
            tb = vbits[k] | (nbits[k] if assume else np.uint32(0))
            with np.errstate(over="ignore"):
                for l in range(L):
                    if l >= 4 and not (int(tb) >> (l - 4)) & 1:
                        continue
                    base = raw[l, k] if (l < 4 or (int(rp[k]) >> (l - 4)) & 1) else 0
                    raw[l, k] = base - dv[l, k] + (dn[l, k] if assume else 0)
            rp[k] |= tb
        keep = alive
    else:
        keep = prep.valid
    kn, kc = np.nonzero(keep)
    return dict(res=out, req=raw, pres=rp, bound_id=prep.id[kn, kc].astype(np.uint32), bound_node=kn.astype(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------
# scenes and the conditions that keep random tests from passing vacuously
# ------------------------------------------------------------------------------------------------------------------------------
PDB_LEVELS = np.array([0, 1, 2, 3, 5, 8, 13, 100, 1000, 5000], np.int64)   # many distinct victim priorities below the preemptors'


def pdb_scene(seed: int, n: int, per_node, S: int, q: int, groups: int, share: float, p: int | None = None, **kw) -> tuple:
    """(scene, bits): preempt_scenes.random_scene tuned so that the bits matter — a spread of victim priorities, preemptors whose cpu
    request needs several victims, few flagged nodes, distinct preemptors (a plan nominates a pod once).  groups == 0: nobody is
    grouped (no policy refusals)."""
    from preempt_scenes import random_scene
    p = p or max(2 * q, 40)
    kw.setdefault("fit_density", 0.8)
    kw.setdefault("flagged", 0.02)
    sc = random_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=max(groups, 1), p=p, protected_share=0.2 if groups else 0.0, levels=PDB_LEVELS, **kw)
    if not groups:
        sc["bound"].group[:] = pr.NOT_GROUPED
        sc["pods"].group[:] = pr.NOT_GROUPED
    rng = np.random.default_rng(seed ^ 0x9DB)
    sc["pod_index"] = rng.permutation(p)[:q].astype(np.uint32)
    sc["pods"].req[0] *= rng.choice([1, 2, 4], size=p)
    # a third of the queue asks for a large part of a node: many potential victims of several priorities have to go, so mixed bits reorder the list
    al = np.sort(sc["nodes"].allocatable[0])
    big = rng.random(p) < 0.35
    sc["pods"].req[0] = np.where(big, (al[rng.integers(0, n, size=p)] * rng.choice([0.4, 0.6, 0.8, 0.95], size=p)).astype(np.int64), sc["pods"].req[0])
    sc["pods"].req[1] = np.where(big, 0, sc["pods"].req[1])
    sc["pods"].req[2] = np.where(big, 0, sc["pods"].req[2])
    sc["priority"] = np.where(rng.random(q) < 0.7, 5000, sc["priority"]).astype(np.int32)
    return sc, pdb_bits(seed, sc["bound"], share)


def pdb_bits(seed: int, bound, share: float) -> np.ndarray:
    """seeded bits: `share` of the bound pods are violating"""
    return (np.random.default_rng(seed ^ 0x9DB).random(bound.b) < share).astype(np.uint8)


def effects(sc: dict, res: dict, plain: dict, bits) -> set:
    """which PDB effects the result `res` (with bits) shows against `plain` (the bits-cleared answer of the same scene)"""
    seen = set()
    b = sc["bound"]
    cap = res["victims"].shape[1]
    for i in range(len(res["node"])):
        if any(not np.array_equal(res[f][i], plain[f][i] if f in plain else 0) for f in FIELDS):
            seen.add("changed")
        if res["node"][i] != plain["node"][i]:
            seen.add("node_differs")
        if res["node"][i] < 0 or res["n_victims"][i] == 0:
            continue
        if res["n_pdb_violations"][i] > 0:
            seen.add("violations_on_chosen")
        nv = int(res["n_victims"][i])
        if nv > cap:
            continue
        v, p = res["victims"][i, :nv], plain["victims"][i, : min(int(plain["n_victims"][i]), cap)]
        if res["node"][i] == plain["node"][i] and sorted(v) == sorted(p) and list(v) != list(p):
            seen.add("order_differs")
        if int(res["top_priority"][i]) < int(b.priority[v].max()):
            seen.add("top_below_max")
        if int(res["earliest_start"][i]) != int(b.start_ns[v[0]]):
            seen.add("est_not_first")
    return seen


EFFECTS = ("node_differs", "order_differs", "violations_on_chosen", "top_below_max", "est_not_first")


def pdb_kats():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preempt_pdb_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_pdb_scene(sc: dict) -> dict:
    from preempt_commit_scenes import kat_commit_scene
    s = kat_commit_scene(sc)
    s["violating"] = np.array(sc["violating"], np.uint8)
    return s


def check_pdb_kat(got: dict, sc: dict, where: str):
    """got: a commit result dict (res, ...) against the scene's hand-derived rows"""
    res = got["res"]
    for i, e in enumerate(sc["expect"]):
        assert int(res["node"][i]) == e["node"], f"{where} [{i}]: node {res['node'][i]} != {e['node']}"
        assert int(res["n_candidates"][i]) == e["n_candidates"], f"{where} [{i}]: n_candidates {res['n_candidates'][i]}"
        assert list(pr.victims_of(res, i)) == e["victims"], f"{where} [{i}]: victims {pr.victims_of(res, i)} != {e['victims']}"
        assert int(res["n_victims"][i]) == e.get("n_victims", len(e["victims"])), f"{where} [{i}]: n_victims {res['n_victims'][i]}"
        assert int(res["n_pdb_violations"][i]) == e["n_pdb_violations"], f"{where} [{i}]: n_pdb_violations {res['n_pdb_violations'][i]}"
        for f in ("top_priority", "priority_sum", "earliest_start"):
            if e[f] is not None:
                assert int(res[f][i]) == e[f], f"{where} [{i}]: {f} {res[f][i]} != {e[f]}"
