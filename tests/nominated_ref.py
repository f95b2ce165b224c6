"""CPU restatements of the resident nominated-pod table and of rule N (include/bsched.h): pods nominated by earlier cycles count in every
fit test of the victim search.  Everything is built ON the existing references by import (tests/preempt_ref.py, preempt_commit_ref.py,
preempt_pdb_ref.py, preempt_gang_ref.py); none of them is edited.

The table, written from the header:
  NomTable      array model: load / apply / read, ids, refusals (NomRefused carries the C error name).
  rebuild_rows  the same history object by object (a list of dicts), what NomTable is held against.

Rule N, two statements:
  object level  run_nom_obj: preempt_ref._add_pod of the qualifying rows in front of the PDB-aware select_victims_on_node.
                plan_nom_obj: the header's slot-walk statement inside a restated slot loop (commit_pdb_obj's and gang_obj's loop): before the
                first slot whose priority is <= a row's priority the row is added to its node exactly as an earlier slot's nominee is;
                the rows never reach the state BS_PREEMPT_APPLY writes.
  array level   run_nom_np / commit_nom_np / gang_nom_np: per-fit-test sums — the [L, n] sum of the rows with priority >= P is added to
                the requests preempt_pdb_ref._eval sees, slot by slot; the working deltas never hold it.
A `rows` argument is the dict NomTable.read() returns (or None: no table)."""
from __future__ import annotations

import copy
import functools

import numpy as np

import preempt_commit_ref as pc
import preempt_gang_ref as gr
import preempt_pdb_ref as pp
import preempt_ref as pr

NOM_MAX, NOM_IDS = 1 << 16, 1 << 24
NONE = 0xFFFFFFFF


class NomRefused(Exception):
    def __init__(self, code: str, why: str):
        super().__init__(f"{code}: {why}")
        self.code = code


def _stored(req, pres, S: int):
    """the lanes as the table stores them: lanes 0..2 the request, the pods lane 1, a scalar lane the request where the bit is set"""
    L = 4 + S
    req = np.asarray(req, np.int64).reshape(L, -1).copy()
    pres = np.asarray(pres, np.uint32).reshape(-1) & np.uint32((1 << S) - 1)
    req[3] = 1
    for s in range(S):
        req[4 + s] = np.where((pres >> np.uint32(s)) & 1, req[4 + s], 0)
    return req, pres


class NomTable:
    """the table as arrays; every refusal is found before anything changes"""

    def __init__(self, S: int):
        self.S, self.L = S, 4 + S
        self.loaded = False

    def load(self, n: int, node, priority, req, pres, m=None):
        node = np.asarray(node, np.uint32).reshape(-1)
        m = node.size if m is None else m
        if m > NOM_MAX:
            raise NomRefused("BS_ERR_CAPACITY", "rows")
        if m and np.any(node >= n):
            raise NomRefused("BS_ERR_INVALID", "node")
        self.n = n
        self.id = np.arange(m, dtype=np.uint32)
        self.node = node.copy()
        self.prio = np.asarray(priority, np.int32).reshape(-1).copy()
        self.req, self.pres = _stored(req if m else np.zeros((self.L, 0)), pres if m else np.zeros(0), self.S)
        self.ids = m
        self.loaded = True

    def apply(self, remove, pod_index, node, priority, pods, n_now=None, max_rows=NOM_MAX, max_ids=NOM_IDS) -> int:
        if not self.loaded:
            raise NomRefused("BS_ERR_STATE", "no table")
        if n_now is not None and n_now != self.n:
            raise NomRefused("BS_ERR_STATE", "stale node count")
        remove = np.asarray(remove, np.uint32).reshape(-1)
        pod_index, node = np.asarray(pod_index, np.uint32).reshape(-1), np.asarray(node, np.uint32).reshape(-1)
        priority = np.asarray(priority, np.int32).reshape(-1)
        if pod_index.size and pods is None:
            raise NomRefused("BS_ERR_STATE", "pods not loaded")
        if np.any(remove >= self.ids):
            raise NomRefused("BS_ERR_INVALID", "unknown id")
        if np.unique(remove).size != remove.size:
            raise NomRefused("BS_ERR_INVALID", "repeated id")
        if not np.all(np.isin(remove, self.id)):
            raise NomRefused("BS_ERR_INVALID", "dead id")
        if pod_index.size and (np.any(pod_index >= pods.p) or np.any(node >= self.n)):
            raise NomRefused("BS_ERR_INVALID", "pod index or node")
        if self.id.size - remove.size + pod_index.size > max_rows:
            raise NomRefused("BS_ERR_CAPACITY", "rows")
        if self.ids + pod_index.size > max_ids:
            raise NomRefused("BS_ERR_CAPACITY", "ids")
        keep = ~np.isin(self.id, remove)
        first = self.ids
        ireq, ipres = _stored(pods.req[: self.L, pod_index], pods.req_present[pod_index], self.S) if pod_index.size else _stored(np.zeros((self.L, 0)), np.zeros(0), self.S)
        self.id = np.concatenate([self.id[keep], first + np.arange(pod_index.size, dtype=np.uint32)]).astype(np.uint32)
        self.node = np.concatenate([self.node[keep], node]).astype(np.uint32)
        self.prio = np.concatenate([self.prio[keep], priority]).astype(np.int32)
        self.pres = np.concatenate([self.pres[keep], ipres]).astype(np.uint32)
        self.req = np.concatenate([self.req[:, keep], ireq], axis=1)
        self.ids = first + pod_index.size
        return first

    def read(self) -> dict:
        return dict(id=self.id.copy(), node=self.node.copy(), priority=self.prio.copy(), req=self.req.copy(), req_present=self.pres.copy())


def rebuild_rows(S: int, history: list, pods) -> list:
    """the table after `history` — [("load", node, priority, req, pres) | ("apply", remove, pod_index, node, priority)] — as row objects;
    only accepted calls are listed"""
    rows, ids = [], 0
    for h in history:
        if h[0] == "load":
            _, node, priority, req, pres = h
            req = np.asarray(req, np.int64).reshape(4 + S, -1)
            rows = [_row_obj(i, int(node[i]), int(priority[i]), [int(req[j, i]) for j in range(4 + S)], int(pres[i]), S) for i in range(len(node))]
            ids = len(node)
        else:
            _, remove, pod_index, node, priority = h
            gone = {int(x) for x in remove}
            rows = [r for r in rows if r["id"] not in gone]
            for k, pi in enumerate(pod_index):
                rows.append(_row_obj(ids + k, int(node[k]), int(priority[k]), [int(pods.req[j, int(pi)]) for j in range(4 + S)],
                                     int(pods.req_present[int(pi)]), S))
            ids += len(pod_index)
    return rows


def _row_obj(i, node, prio, req, pres, S) -> dict:
    return {"id": i, "node": node, "priority": prio, "req": req[:3], "scalar": {s: req[4 + s] for s in range(S) if (pres >> s) & 1}}


def rows_as_objects(rows: dict | None, S: int) -> list:
    if rows is None:
        return []
    return [_row_obj(int(rows["id"][i]), int(rows["node"][i]), int(rows["priority"][i]), [int(rows["req"][j, i]) for j in range(4 + S)],
                     int(rows["req_present"][i]), S) for i in range(len(rows["id"]))]


def objects_as_rows(objs: list, S: int) -> dict:
    m = len(objs)
    req = np.zeros((4 + S, m), np.int64)
    pres = np.zeros(m, np.uint32)
    for i, r in enumerate(objs):
        req[:3, i] = r["req"]
        req[3, i] = 1
        for s, v in r["scalar"].items():
            req[4 + s, i] = v
            pres[i] |= np.uint32(1 << s)
    return dict(id=np.array([r["id"] for r in objs], np.uint32), node=np.array([r["node"] for r in objs], np.uint32),
                priority=np.array([r["priority"] for r in objs], np.int32), req=req, req_present=pres)


# ------------------------------------------------------------------------------------------------------------------------------
# rule N, object level
# ------------------------------------------------------------------------------------------------------------------------------
def _add_row(state, row: dict, S: int):
    """addNominatedPods for one row: AddPod on the node's NodeInfo"""
    ni = pr._node_info(state, row["node"], S)
    pr._add_pod(ni, row)
    state.put(row["node"], ni)


def run_nom_obj(nodes, fit, pods, bound, S, pod_index, priority, protected, cap, violating, rows) -> dict:
    """bs_preempt_run: every preemptor on its own, the rows of priority >= its own added in front of the search"""
    violating = gr._bits(bound, violating)
    per = pr.bound_objects(bound, S)
    fitb = fit.to_bool()
    objs = rows_as_objects(rows, S)
    out = pp._empty(len(pod_index), cap)
    for i in range(len(pod_index)):
        pi, P = int(pod_index[i]), int(priority[i])
        req = [int(pods.req[j, pi]) for j in range(4 + S)]
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        state = pc._NodeState(nodes)
        for r in objs:
            if r["priority"] >= P:                       # GetPodPriority(p) >= GetPodPriority(pod)
                _add_row(state, r, S)
        nv, viol = pp._search_obj(state, fitb, per, req, pres, cls, grp, P, protected, S, violating)
        out["n_candidates"][i] = len(nv)
        node = pp.pick_one_node(nv, viol)
        if node is not None:
            pp._fill(out, i, node, nv[node], viol[node], cap)
    return out


def plan_nom_obj(nodes, fit, pods, bound, S, pod_index, priority, protected, cap, violating, rows, need=None, apply=False, assume=False) -> dict:
    """bs_preempt_commit (need None) and bs_preempt_commit_gang: gang_obj's slot loop restated, with the header's slot walk — a row
    enters the WORKING state before the first slot whose priority is <= its own, as an earlier slot's nominee does; `final`, what
    APPLY writes, never sees a row.  A voided run is restored from its snapshot; the rows that entered inside it stay."""
    violating = gr._bits(bound, violating)
    need = np.zeros(0, np.int64) if need is None else np.asarray(need, np.int64).reshape(-1)
    per = pr.bound_objects(bound, S)
    for k in per:
        per[k].sort(key=functools.cmp_to_key(pr._more_important))
    work, final = pc._NodeState(nodes), pc._NodeState(nodes)
    fitb = fit.to_bool()
    q = len(pod_index)
    out = pp._empty(q, cap)
    voided, placed_of = np.zeros(q, np.uint8), np.zeros(need.size, np.uint32)
    order = pc.slot_order(priority)
    runs = gr.runs_of([int(pods.group[int(pod_index[i])]) for i in order], need)
    start_of = {s: (e, g) for s, e, g in runs}
    end_of = {e: (s, g) for s, e, g in runs}
    waiting = sorted(rows_as_objects(rows, S), key=lambda r: -r["priority"])     # the rows not added yet, highest priority first
    snap, since = None, []
    for s, i in enumerate(order):
        pi, P = int(pod_index[i]), int(priority[i])
        while waiting and waiting[0]["priority"] >= P:                           # the slot walk
            r = waiting.pop(0)
            _add_row(work, r, S)
            since.append(r)
        if s in start_of:
            snap = (copy.deepcopy(per), work.requested.copy(), work.requested_present.copy(), final.requested.copy(),
                    final.requested_present.copy())
            since = []
        req = [int(pods.req[j, pi]) for j in range(4 + S)]
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        nv, viol = pp._search_obj(work, fitb, per, req, pres, cls, grp, P, protected, S, violating)
        out["n_candidates"][i] = len(nv)
        node = pp.pick_one_node(nv, viol)
        if node is not None:
            v = nv[node]
            pp._fill(out, i, node, v, viol[node], cap)
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
        if s in end_of:
            s0, g = end_of[s]
            members = [int(x) for x in order[s0:s + 1]]
            placed = sum(1 for m in members if out["node"][m] >= 0)
            placed_of[g] = placed
            if placed < int(need[g]):
                per = snap[0]
                work.requested, work.requested_present = snap[1], snap[2]
                final.requested, final.requested_present = snap[3], snap[4]
                for r in since:                                                  # rows are not the run's: they stay
                    _add_row(work, r, S)
                for m in members:
                    if out["node"][m] >= 0:
                        voided[m] = 1
                        out["node"][m] = -1
                        out["n_victims"][m] = 0
                        out["victims"][m, :] = 0
                        for f in ("top_priority", "priority_sum", "earliest_start", "n_pdb_violations"):
                            out[f][m] = 0
            snap = None
    if not apply:
        final = pc._NodeState(nodes)
        per = pr.bound_objects(bound, S)
        for k in per:
            per[k].sort(key=functools.cmp_to_key(pr._more_important))
    ids = [p["id"] for k in sorted(per) for p in per[k]]
    nodes_of = [k for k in sorted(per) for _ in per[k]]
    return dict(res=out, req=final.requested, pres=final.requested_present, bound_id=np.array(ids, np.uint32),
                bound_node=np.array(nodes_of, np.uint32), slot_voided=voided, group_placed=placed_of)


# ------------------------------------------------------------------------------------------------------------------------------
# rule N, array level: per-fit-test sums
# ------------------------------------------------------------------------------------------------------------------------------
class NomSums:
    """sum(P) [L, n]: the stored lanes of every row with priority >= P, wrapping"""

    def __init__(self, rows: dict | None, L: int, n: int):
        self.L, self.n, self.rows = L, n, rows

    def __call__(self, P: int) -> np.ndarray:
        out = np.zeros((self.L, self.n), np.int64)
        if self.rows is None or not len(self.rows["id"]):
            return out
        sel = self.rows["priority"].astype(np.int64) >= P
        with np.errstate(over="ignore"):
            for l in range(self.L):
                np.add.at(out[l], self.rows["node"][sel].astype(np.int64), self.rows["req"][l, sel])
        return out


def run_nom_np(prep: "pp.PdbPrep", fit, pods, pod_index, priority, protected, cap, rows) -> dict:
    fitb, prot = pp._common(prep, fit, protected)
    sums = NomSums(rows, prep.L, prep.N)
    out = pp._empty(len(pod_index), cap)
    allcols = np.arange(prep.N)
    for i in range(len(pod_index)):
        pi, P = int(pod_index[i]), int(priority[i])
        req = pods.req[: prep.L, pi].astype(np.int64)
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        with np.errstate(over="ignore"):
            cur = prep.cur0 + sums(P)
        cand, victim = pp._eval(prep, allcols, prep.valid, cur, req, pres, cls, grp, P, fitb, prot)
        pp._pick(prep, cand, victim, out, i, cap)
    return out


def commit_nom_np(prep: "pp.PdbPrep", fit, pods, bound, pod_index, priority, protected, cap, rows, apply=False, assume=False) -> dict:
    """commit_pdb_np's loop with sum(P) on top of the requests both evaluations see; dv / dn / raw never hold it"""
    S, L, N = prep.S, prep.L, prep.N
    fitb, prot = pp._common(prep, fit, protected)
    sums = NomSums(rows, L, N)
    alive = prep.valid.copy()
    cur = prep.cur0.copy()
    dv, dn = np.zeros((L, N), np.int64), np.zeros((L, N), np.int64)
    vbits, nbits = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    touched = np.zeros(N, bool)
    bpres = np.zeros((N, prep.M), np.uint32)
    bpres[prep.valid] = bound.req_present[prep.id[prep.valid]]
    smask = np.uint32((1 << S) - 1)
    q = len(pod_index)
    out = pp._empty(q, cap)
    allcols = np.arange(N)
    for i in pc.slot_order(priority):
        pi, P = int(pod_index[i]), int(priority[i])
        req = pods.req[:L, pi].astype(np.int64)
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        with np.errstate(over="ignore"):
            add = sums(P)
            c1, v1 = pp._eval(prep, allcols[~touched], prep.valid, prep.cur0 + add, req, pres, cls, grp, P, fitb, prot)
            c2, v2 = pp._eval(prep, allcols[touched], alive, cur + add, req, pres, cls, grp, P, fitb, prot)
        cand, victim = np.concatenate([c1, c2]), np.concatenate([v1, v2])
        o = np.argsort(cand, kind="stable")
        k, vm = pp._pick(prep, cand[o], victim[o], out, i, cap)
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


def gang_nom_np(prep: "pp.PdbPrep", fit, pods, bound, pod_index, priority, protected, need, cap, rows, apply=False, assume=False) -> dict:
    """the defining property of bs_preempt_commit_gang (preempt_gang_ref.survivors / gang_np) over commit_nom_np"""
    need = np.asarray(need, np.int64).reshape(-1)
    pod_index, priority = np.asarray(pod_index), np.asarray(priority)
    order = pc.slot_order(priority)
    runs = gr.runs_of([int(pods.group[int(pod_index[i])]) for i in order], need)
    q = len(order)
    voided, placed_of, saw = np.zeros(q, np.uint8), np.zeros(need.size, np.uint32), {}
    keep, s = [], 0
    for s0, e, g in runs:
        keep += [int(x) for x in order[s:s0]]
        members = [int(x) for x in order[s0:e + 1]]
        trial = keep + members
        r = commit_nom_np(prep, fit, pods, bound, pod_index[trial], priority[trial], protected, cap, rows)["res"]
        got = r["node"][len(keep):] >= 0
        placed_of[g] = int(got.sum())
        if placed_of[g] >= need[g]:
            keep += members
        else:
            for j, m in enumerate(members):
                voided[m] = 1 if got[j] else 0
                saw[m] = int(r["n_candidates"][len(keep) + j])
        s = e + 1
    keep += [int(x) for x in order[s:]]
    sub = commit_nom_np(prep, fit, pods, bound, pod_index[keep], priority[keep], protected, cap, rows, apply, assume)
    out = pp._empty(q, cap)
    for f in pp.FIELDS:
        if keep:
            out[f][keep] = sub["res"][f]
    for m, c in saw.items():
        out["n_candidates"][m] = c
    return dict(res=out, req=sub["req"], pres=sub["pres"], bound_id=sub["bound_id"], bound_node=sub["bound_node"], slot_voided=voided,
                group_placed=placed_of)


def nominate_rows(table: NomTable, res: dict, pod_index, priority, pods) -> np.ndarray:
    """BS_PREEMPT_NOMINATE on the model: every preemptor that holds a node is appended in the caller's order; returns the id per preemptor"""
    node = np.asarray(res["node"])
    has = node >= 0
    ids = np.full(node.size, NONE, np.uint32)
    first = table.apply([], np.asarray(pod_index)[has], node[has].astype(np.uint32), np.asarray(priority)[has], pods)
    ids[has] = first + np.arange(int(has.sum()), dtype=np.uint32)
    return ids


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------------------
def nom_rows_for(sc: dict, seed: int, density: float = 0.6, per_node=(1, 3)) -> dict:
    """rows for a scene: `density` of the nodes hold 1..3 rows; priorities straddle the preemptors' (each one's own, one below, one above);
    requests are those of queue pods (cpu scaled so that a row often decides a fit test)"""
    rng = np.random.default_rng(seed ^ 0x40B)
    S, n, pods = sc["S"], sc["nodes"].n, sc["pods"]
    hold = np.nonzero(rng.random(n) < density)[0]
    node = np.repeat(hold, rng.integers(per_node[0], per_node[1] + 1, size=hold.size)).astype(np.uint32)
    m = node.size
    base = np.asarray(sc["priority"], np.int64)
    prio = (base[rng.integers(0, base.size, size=m)] + rng.integers(-1, 2, size=m)).astype(np.int32) if base.size else np.zeros(m, np.int32)
    src = rng.integers(0, pods.p, size=m)
    req = pods.req[: 4 + S, src].astype(np.int64).copy()
    free = (sc["nodes"].allocatable[0] - sc["nodes"].requested[0])[node]
    req[0] = np.where(rng.random(m) < 0.5, np.maximum(free, 0) // 2 + req[0], req[0])
    t = NomTable(S)
    t.load(n, node, prio, req, pods.req_present[src])
    return t.read()


def changed(a: dict, b: dict) -> bool:
    """the table changes an answer: the node, the victim list or the pick key of some preemptor"""
    return any(not np.array_equal(a[f], b[f]) for f in ("node", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start", "n_pdb_violations"))
