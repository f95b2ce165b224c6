"""Two independent CPU restatements of bs_preempt_commit_gang (include/bsched.h): bs_preempt_commit with each gang's quorum decided
inside the pass, built on tests/preempt_commit_ref.py and tests/preempt_pdb_ref.py by import (the PDB-aware search: all-zero bits give
the plain one).

  gang_obj   object level: tests/preempt_pdb_ref.py's sequential loop over per-node pod lists and NodeInfo-like dicts; at a run's first
             slot it snapshots the lists and the node state, and after the run's last slot it puts them back when the run missed its
             quorum.  Also returns the trace of every run (what its slots answered BEFORE the decision), for tests/preempt_gang_paths.py.
  gang_np    the defining property, literally: the runs are decided in slot order (a run is answered after the preemptors that survive
             so far, by commit_pdb_np, plan only), then commit_pdb_np answers the list without the voided runs' preemptors.

Both return preempt_pdb_ref's dict (res with n_pdb_violations, req, pres, bound_id, bound_node) plus slot_voided [count] (uint8) and
group_placed [g] (uint32).  A group that forms a second run raises RunError (the library answers BS_ERR_INVALID)."""
from __future__ import annotations

import copy
import functools

import numpy as np

import preempt_commit_ref as pc
import preempt_pdb_ref as pp
import preempt_ref as pr


class RunError(ValueError):
    pass


def runs_of(slot_groups, need) -> list:
    """the runs of a slot list: [(first slot, last slot, group)], slots in slot order; RunError where a group forms two"""
    need = np.asarray(need, np.int64).reshape(-1)
    out, seen, s, q = [], set(), 0, len(slot_groups)
    while s < q:
        g = int(slot_groups[s])
        if g < 0 or g >= need.size or need[g] <= 0:
            s += 1
            continue
        if g in seen:
            raise RunError(f"group {g} forms a second run at slot {s}")
        e = s
        while e + 1 < q and int(slot_groups[e + 1]) == g:
            e += 1
        out.append((s, e, g))
        seen.add(g)
        s = e + 1
    return out


def gang_order(pod_group, priority) -> np.ndarray:
    """restates capi.gang_order: priority descending, then first appearance of the group at that priority, then the caller's order"""
    idx = list(range(len(priority)))
    first = {}
    for i in idx:
        key = (int(priority[i]), int(pod_group[i])) if pod_group[i] >= 0 else (int(priority[i]), "solo", i)
        first.setdefault(key, i)
    keyf = lambda i: (-int(priority[i]), first[(int(priority[i]), int(pod_group[i])) if pod_group[i] >= 0 else (int(priority[i]), "solo", i)], i)
    return np.array(sorted(idx, key=keyf), np.int64)


def _bits(bound, violating):
    return np.zeros(max(bound.b, 1), np.uint8) if violating is None else np.asarray(violating, np.uint8).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------------
# object level: snapshot at a run's start, restore on a miss
# ------------------------------------------------------------------------------------------------------------------------------
def gang_obj(nodes, fit, pods, bound, S, pod_index, priority, protected, need, cap, apply=False, assume=False, violating=None) -> dict:
    violating = _bits(bound, violating)
    need = np.asarray(need, np.int64).reshape(-1)
    per = pr.bound_objects(bound, S)
    for k in per:
        per[k].sort(key=functools.cmp_to_key(pr._more_important))
    work, final = pc._NodeState(nodes), pc._NodeState(nodes)
    fitb = fit.to_bool()
    q = len(pod_index)
    out = pp._empty(q, cap)
    voided, placed_of = np.zeros(q, np.uint8), np.zeros(need.size, np.uint32)
    order = pc.slot_order(priority)
    runs = runs_of([int(pods.group[int(pod_index[i])]) for i in order], need)
    start_of = {s: (e, g) for s, e, g in runs}
    end_of = {e: (s, g) for s, e, g in runs}
    trace, snap, answered = [], None, {}
    for s, i in enumerate(order):
        if s in start_of:
            snap = (copy.deepcopy(per), work.requested.copy(), work.requested_present.copy(), final.requested.copy(),
                    final.requested_present.copy())
        pi, P = int(pod_index[i]), int(priority[i])
        req = [int(pods.req[j, pi]) for j in range(4 + S)]
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        nv, viol = pp._search_obj(work, fitb, per, req, pres, cls, grp, P, protected, S, violating)
        out["n_candidates"][i] = len(nv)
        node = pp.pick_one_node(nv, viol)
        answered[int(i)] = dict(preemptor=int(i), node=-1, victims=[], n_pdb_violations=0)
        if node is not None:
            v = nv[node]
            pp._fill(out, i, node, v, viol[node], cap)
            answered[int(i)] = dict(preemptor=int(i), node=int(node), victims=[p["id"] for p in v], n_pdb_violations=int(viol[node]) if v else 0)
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
            void = placed < int(need[g])
            trace.append(dict(group=g, first=s0, last=s, need=int(need[g]), placed=placed, voided=void,
                              slots=[answered[m] for m in members]))
            if void:
                per = snap[0]
                work.requested, work.requested_present = snap[1], snap[2]
                final.requested, final.requested_present = snap[3], snap[4]
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
                bound_node=np.array(nodes_of, np.uint32), slot_voided=voided, group_placed=placed_of, trace=trace, answered=answered)


# ------------------------------------------------------------------------------------------------------------------------------
# the defining property
# ------------------------------------------------------------------------------------------------------------------------------
def survivors(prep, fit, pods, bound, pod_index, priority, protected, need, cap):
    """the runs decided in slot order: (caller indices of the preemptors that are not in a voided run, in slot order; slot_voided;
    group_placed; {caller index: n_candidates a voided run's slot saw})"""
    need = np.asarray(need, np.int64).reshape(-1)
    pod_index, priority = np.asarray(pod_index), np.asarray(priority)
    order = pc.slot_order(priority)
    runs = runs_of([int(pods.group[int(pod_index[i])]) for i in order], need)
    q = len(order)
    voided, placed_of, saw = np.zeros(q, np.uint8), np.zeros(need.size, np.uint32), {}
    keep, s = [], 0
    for s0, e, g in runs:
        keep += [int(x) for x in order[s:s0]]
        members = [int(x) for x in order[s0:e + 1]]
        trial = keep + members                              # slot order already: the stable sort inside keeps it
        r = pp.commit_pdb_np(prep, fit, pods, bound, pod_index[trial], priority[trial], protected, cap)["res"]
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
    return keep, voided, placed_of, saw


def gang_np(prep: "pp.PdbPrep", fit, pods, bound, pod_index, priority, protected, need, cap, apply=False, assume=False) -> dict:
    pod_index, priority = np.asarray(pod_index), np.asarray(priority)
    keep, voided, placed_of, saw = survivors(prep, fit, pods, bound, pod_index, priority, protected, need, cap)
    q = len(pod_index)
    sub = pp.commit_pdb_np(prep, fit, pods, bound, pod_index[keep], priority[keep], protected, cap, apply, assume)
    out = pp._empty(q, cap)
    for f in pp.FIELDS:
        if keep:
            out[f][keep] = sub["res"][f]
    for m, c in saw.items():
        out["n_candidates"][m] = c
    return dict(res=out, req=sub["req"], pres=sub["pres"], bound_id=sub["bound_id"], bound_node=sub["bound_node"], slot_voided=voided,
                group_placed=placed_of, keep=keep)
