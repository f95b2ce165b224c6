"""Two independent CPU restatements of bs_preempt_commit (include/bsched.h): the preemptors answered in sequence, each slot seeing the
earlier slots' victims gone (removed from the bound lists, NodeInfo.RemovePod on the node) and their preemptors nominated on their
nodes (AddPod), built on tests/preempt_ref.py's functions.

  commit_obj  object level: per-node pod lists and NodeInfo-like dicts, a loop over preempt_ref.select_victims_on_node /
              pick_one_node that mutates them.
  commit_np   numpy: the base state's arrays (preempt_ref.Prep) for clean nodes, working arrays re-evaluated for the touched nodes only.

Both return dict(res=<the dict Context.preempt returns>, req=[L, n] final node requests, pres=[n] final present bits, bound_id=[b'],
bound_node=[b']: the surviving bound table in table order).  The final state is what the flags leave: unchanged for a plan only,
victims removed for apply, nominees added as well for assume."""
from __future__ import annotations

import functools

import numpy as np

import preempt_ref as pr

NOT_GROUPED, GROUP_MISSING, MAX_INT32 = pr.NOT_GROUPED, pr.GROUP_MISSING, pr.MAX_INT32


def slot_order(priority) -> np.ndarray:
    """priority descending, equal priorities in the caller's order"""
    return np.argsort(-np.asarray(priority, np.int64), kind="stable")


# ------------------------------------------------------------------------------------------------------------------------------
# object level
# ------------------------------------------------------------------------------------------------------------------------------
class _NodeState:
    """the node columns preempt_ref reads (allocatable, requested, present bits, flags), with requests of our own to mutate"""

    def __init__(self, nodes):
        self.n = nodes.n
        self.allocatable, self.allocatable_present, self.flags = nodes.allocatable, nodes.allocatable_present, nodes.flags
        self.requested = np.array(nodes.requested, np.int64, copy=True)
        self.requested_present = np.array(nodes.requested_present, np.uint32, copy=True)

    def put(self, k: int, ni: dict):
        """write a NodeInfo dict back: lanes 0..3, and every scalar key the dict holds (the key becomes present)"""
        for j, name in enumerate(("cpu", "mem", "eph", "pods")):
            self.requested[j, k] = ni[name]
        for s, v in ni["scalar"].items():
            self.requested[4 + s, k] = v
            self.requested_present[k] |= np.uint32(1 << s)


def _pod_obj(pods, pi: int, S: int) -> dict:
    return {"req": [int(pods.req[j, pi]) for j in range(3)],
            "scalar": {s: int(pods.req[4 + s, pi]) for s in range(S) if (int(pods.req_present[pi]) >> s) & 1}}


def commit_obj(nodes, fit, pods, bound, S, pod_index, priority, protected, cap, apply=False, assume=False) -> dict:
    per = pr.bound_objects(bound, S)
    for k in per:
        per[k].sort(key=functools.cmp_to_key(pr._more_important))
    work, final = _NodeState(nodes), _NodeState(nodes)
    fitb = fit.to_bool()
    q = len(pod_index)
    out = pr._empty(q, cap)
    for i in slot_order(priority):
        pi, P = int(pod_index[i]), int(priority[i])
        req = [int(pods.req[j, pi]) for j in range(4 + S)]
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        nv = {}
        for k in range(nodes.n):
            if nodes.flags[k] or cls >= fitb.shape[0] or not fitb[cls, k]:
                continue
            victims, ok = pr.select_victims_on_node(work, k, per.get(k, []), req, pres, grp, P, protected, S)
            if ok:
                nv[k] = victims
        out["n_candidates"][i] = len(nv)
        node = pr.pick_one_node(nv)
        if node is None:
            continue
        v = nv[node]
        out["node"][i] = node
        out["n_victims"][i] = len(v)
        for j, p in enumerate(v[:cap]):
            out["victims"][i, j] = p["id"]
        if v:
            out["top_priority"][i] = v[0]["priority"]
            out["priority_sum"][i] = sum(p["priority"] + (MAX_INT32 + 1) for p in v)
            out["earliest_start"][i] = pr.earliest_start(v)
        # the commit: the victims leave the node's list and its requests, the preemptor is nominated on it
        gone = {p["id"] for p in v}
        per[node] = [p for p in per.get(node, []) if p["id"] not in gone]
        nom = _pod_obj(pods, pi, S)
        for st, add in ((work, True), (final, assume)):
            ni = pr._node_info(st, node, S)
            for p in v:
                pr._remove_pod(ni, p)
            if add:
                pr._add_pod(ni, nom)
            st.put(node, ni)
    if not apply:
        final = _NodeState(nodes)
        per = pr.bound_objects(bound, S)
        for k in per:
            per[k].sort(key=functools.cmp_to_key(pr._more_important))
    ids = [p["id"] for k in sorted(per) for p in per[k]]
    nodes_of = [k for k in sorted(per) for _ in per[k]]
    return dict(res=out, req=final.requested, pres=final.requested_present, bound_id=np.array(ids, np.uint32),
                bound_node=np.array(nodes_of, np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------
# numpy: base arrays for clean nodes, working arrays for the touched ones
# ------------------------------------------------------------------------------------------------------------------------------
def _eval(prep, cols, valid, cur, req, pres, cls, grp, P, fitb, prot):
    """steps 1-5 on the node columns `cols` with bound-entry mask valid [N, M] and effective requests cur [L, N]:
    (candidate columns in `cols` order, victim mask [c, M])"""
    S = prep.S
    ok = prep.flags[cols] == 0
    ok &= fitb[cls, cols] if cls < fitb.shape[0] else np.zeros(cols.size, bool)
    g = prep.group[cols]
    vm = valid[cols] & (prep.prio[cols] < P)
    q_grouped = grp != NOT_GROUPED
    v_bad = (g == GROUP_MISSING) | ((g >= 0) & prot[np.clip(g, 0, None)])
    bad = np.where(g == NOT_GROUPED, q_grouped, v_bad | (q_grouped & (g == grp)))
    ok &= ~np.any(vm & bad, axis=1)
    with np.errstate(over="ignore"):
        c = cur[:, cols] - (prep.req[:, cols] * vm[None]).sum(axis=2)
    ok &= pr.holds_np(prep.alloc[:, cols], prep.apres[cols], c, req, pres, S)
    sel = np.nonzero(ok)[0]
    cand, m, c = cols[sel], vm[sel], c[:, sel]
    al, ap, rq = prep.alloc[:, cand], prep.apres[cand], prep.req[:, cand]
    victim = np.zeros(m.shape, bool)
    with np.errstate(over="ignore"):
        for col in range(prep.M):
            mc = m[:, col]
            if not mc.any():
                continue
            t = c + rq[:, :, col] * mc[None]
            h = pr.holds_np(al, ap, t, req, pres, S)
            c = np.where((mc & h)[None], t, c)
            victim[:, col] = mc & ~h
    return cand, victim


def commit_np(prep: "CommitPrep", fit, pods, bound, pod_index, priority, protected, cap, apply=False, assume=False) -> dict:
    S, L, N = prep.S, prep.L, prep.N
    fitb = fit.to_bool() if N else np.zeros((0, 0), bool)
    prot = np.asarray(protected, bool) if protected is not None and len(protected) else np.zeros(1, bool)
    alive = prep.valid.copy()
    cur = prep.cur0.copy()                          # effective working requests
    dv, dn = np.zeros((L, N), np.int64), np.zeros((L, N), np.int64)
    vbits, nbits = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    touched = np.zeros(N, bool)
    bpres = np.zeros((N, prep.M), np.uint32)
    bpres[prep.valid] = bound.req_present[prep.id[prep.valid]]
    smask = np.uint32((1 << S) - 1)
    q = len(pod_index)
    out = pr._empty(q, cap)
    allcols = np.arange(N)
    for i in slot_order(priority):
        pi, P = int(pod_index[i]), int(priority[i])
        req = pods.req[:L, pi].astype(np.int64)
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        clean, dirty = allcols[~touched], allcols[touched]
        c1, v1 = _eval(prep, clean, prep.valid, prep.cur0, req, pres, cls, grp, P, fitb, prot)
        c2, v2 = _eval(prep, dirty, alive, cur, req, pres, cls, grp, P, fitb, prot)
        cand = np.concatenate([c1, c2])
        victim = np.concatenate([v1, v2])
        o = np.argsort(cand, kind="stable")
        cand, victim = cand[o], victim[o]
        out["n_candidates"][i] = cand.size
        if cand.size == 0:
            continue
        pr_, st = prep.prio[cand], prep.start[cand]
        nv = victim.sum(axis=1)
        if np.any(nv == 0):
            w = int(np.nonzero(nv == 0)[0][0])
        else:
            first = victim.argmax(axis=1)
            top = pr_[np.arange(cand.size), first]
            est = st[np.arange(cand.size), first]
            ssum = np.where(victim, pr_ + (MAX_INT32 + 1), 0).sum(axis=1)
            w = int(np.lexsort((cand, ~est, nv, ssum, top))[0])
            out["top_priority"][i] = top[w]
            out["priority_sum"][i] = ssum[w]
            out["earliest_start"][i] = est[w]
        k = int(cand[w])
        out["node"][i] = k
        out["n_victims"][i] = nv[w]
        vm = victim[w]
        vid = prep.id[k][vm]
        out["victims"][i, : min(vid.size, cap)] = vid[:cap]
        # the commit
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
    raw = prep.raw_req.copy()
    rp = prep.raw_pres.copy()
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
    kn, kc = np.nonzero(keep)                       # row-major: node ascending, importance order within a node
    return dict(res=out, req=raw, pres=rp, bound_id=prep.id[kn, kc].astype(np.uint32), bound_node=kn.astype(np.uint32))


class CommitPrep(pr.Prep):
    """preempt_ref.Prep plus the raw node requests and present bits (what bs_nodes_read returns)"""

    def __init__(self, nodes, bound, S: int):
        super().__init__(nodes, bound, S)
        self.raw_req = np.array(nodes.requested, np.int64, copy=True)
        self.raw_pres = np.array(nodes.requested_present, np.uint32, copy=True)


def victim_ids(res: dict) -> list:
    return [int(v) for i in range(len(res["node"])) for v in pr.victims_of(res, i)]
