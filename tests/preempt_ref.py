"""Two independent CPU restatements of bs_preempt_run (include/bsched.h): the gang-aware victim search of upstream's preemption
(k8s v1.17.5 generic_scheduler.go: selectVictimsOnNode, pickOneNodeForPreemption) gated by the plugin's PreemptRemovePod
(core.go:197-260).  They live under tests/ because oracle/ is frozen.

  preempt_obj  object level: lists of pod dicts per node, a NodeInfo-like dict per node copy, the three upstream functions written
               out as they read (policy errors as strings, a comparator sort, the pick as its five filtering passes).
  preempt_np   numpy, vectorised over nodes (and over the victims of a node through a mask), for full sizes.

A scene is (nodes: soa.Nodes, fit: soa.FitMasks, pods: soa.Pods, bound: soa.Bound, S); a call adds the preemptors (pod_index,
priority) and group_protected[g].  Both return the dict Context.preempt returns (victims as a [count, cap] array, zero-padded)."""
from __future__ import annotations

import functools

import numpy as np

NOT_GROUPED, GROUP_MISSING = -1, -2
MAX_INT32 = (1 << 31) - 1
MAX_INT64 = (1 << 63) - 1


def _wrap(x: int) -> int:
    """int64 two's-complement wrap (Go arithmetic)"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


# ------------------------------------------------------------------------------------------------------------------------------
# object level
# ------------------------------------------------------------------------------------------------------------------------------
def remove_policy(q_group: int, v_group: int, protected) -> str | None:
    """ScheduleOperation.PreemptRemovePod(podToSchedule=q, podToRemove=v), core.go:203-260: None = allowed, else the error text.
    VerifyPodLabelSatisfied: a pod is "offline" iff it carries the PodGroup label (group index or GROUP_MISSING)."""
    offline_remove = v_group != NOT_GROUPED
    offline_schedule = q_group != NOT_GROUPED
    if not offline_schedule and not offline_remove:                       # :211-213 online preempts online
        return None
    if offline_schedule and not offline_remove:                           # :216-218
        return "offline pods are forbidden to preempt online"

    def check_preemption():                                               # :220-241
        if v_group == GROUP_MISSING:                                      # pgsObj == nil, :223-225
            return "", "can not found pod group"
        if protected[v_group]:                                            # Phase Scheduled / Running, :235-238
            return "", "pod belongs to Scheduled or Running pod group can not be scheduled"
        return ("pg", v_group), None

    full_remove, err = check_preemption()
    if not offline_schedule and offline_remove:                           # :245-247 online preempts offline
        return err
    # offline preempts offline, :250-256: the full names compared; an unknown group of q has a name no known group has
    full_schedule = ("pg", q_group) if q_group >= 0 else ("unknown", q_group)
    if full_remove == full_schedule:
        return "podToSchedule and podToRemove belong to same pod group, do not preempt"
    if err is not None:
        return err
    return None


def _node_info(nodes, k: int, S: int) -> dict:
    """NodeInfo.requestedResource of node k: cpu / mem / eph / pod count and the ScalarResources map (present keys only)"""
    r = nodes.requested
    ni = {"cpu": int(r[0, k]), "mem": int(r[1, k]), "eph": int(r[2, k]), "pods": int(r[3, k]), "scalar": {}}
    for s in range(S):
        if (int(nodes.requested_present[k]) >> s) & 1:
            ni["scalar"][s] = int(r[4 + s, k])
    return ni


def _remove_pod(ni: dict, pod: dict):
    """NodeInfo.RemovePod: the request leaves, the pod count drops by one; scalar keys of the pod are subtracted (absent = 0)"""
    ni["cpu"] = _wrap(ni["cpu"] - pod["req"][0])
    ni["mem"] = _wrap(ni["mem"] - pod["req"][1])
    ni["eph"] = _wrap(ni["eph"] - pod["req"][2])
    ni["pods"] = _wrap(ni["pods"] - 1)
    for s, v in pod["scalar"].items():
        ni["scalar"][s] = _wrap(ni["scalar"].get(s, 0) - v)


def _add_pod(ni: dict, pod: dict):
    ni["cpu"] = _wrap(ni["cpu"] + pod["req"][0])
    ni["mem"] = _wrap(ni["mem"] + pod["req"][1])
    ni["eph"] = _wrap(ni["eph"] + pod["req"][2])
    ni["pods"] = _wrap(ni["pods"] + 1)
    for s, v in pod["scalar"].items():
        ni["scalar"][s] = _wrap(ni["scalar"].get(s, 0) + v)


def holds_obj(nodes, k: int, ni: dict, req, pres: int, S: int) -> bool:
    """oracle/bs_oracle_seq.c:62-78 holds() on the node info `ni`"""
    al = nodes.allocatable
    for j, name in enumerate(("cpu", "mem", "eph")):
        if req[j] > 0 and req[j] > _wrap(int(al[j, k]) - ni[name]):
            return False
    if _wrap(ni["pods"] + 1) > int(al[3, k]):
        return False
    for s in range(S):
        if not ((pres >> s) & 1) or req[4 + s] <= 0:
            continue
        if not ((int(nodes.allocatable_present[k]) >> s) & 1):
            return False
        if req[4 + s] > _wrap(int(al[4 + s, k]) - ni["scalar"].get(s, 0)):
            return False
    return True


def bound_objects(bound, S: int) -> list[list[dict]]:
    """the bound table as NodeInfo.Pods() lists (table order)"""
    per: dict[int, list] = {}
    for i in range(bound.b):
        pod = {"id": i, "priority": int(bound.priority[i]), "start": int(bound.start_ns[i]), "group": int(bound.group[i]),
               "req": [int(bound.req[j, i]) for j in range(3)],
               "scalar": {s: int(bound.req[4 + s, i]) for s in range(S) if (int(bound.req_present[i]) >> s) & 1}}
        per.setdefault(int(bound.node[i]), []).append(pod)
    return per


def _more_important(p1: dict, p2: dict) -> int:
    """util.MoreImportantPod as a comparator (higher priority first, then the earlier start), pod id as the tie rule"""
    if p1["priority"] != p2["priority"]:
        return -1 if p1["priority"] > p2["priority"] else 1
    if p1["start"] != p2["start"]:
        return -1 if p1["start"] < p2["start"] else 1
    return -1 if p1["id"] < p2["id"] else (1 if p1["id"] > p2["id"] else 0)


def select_victims_on_node(nodes, k, pods_on_node, q_req, q_pres, q_group, P, protected, S):
    """selectVictimsOnNode: (victims in importance order, fits)"""
    ni = _node_info(nodes, k, S)
    potential = []
    for p in pods_on_node:
        if p["priority"] < P:
            potential.append(p)
            _remove_pod(ni, p)
            if remove_policy(q_group, p["group"], protected) is not None:
                return None, False
    if not holds_obj(nodes, k, ni, q_req, q_pres, S):
        return None, False
    potential.sort(key=functools.cmp_to_key(_more_important))
    victims = []
    for p in potential:                                  # reprievePod over the non-violating victims (no PDBs)
        _add_pod(ni, p)
        if not holds_obj(nodes, k, ni, q_req, q_pres, S):
            _remove_pod(ni, p)
            victims.append(p)
    return victims, True


def pick_one_node(nodes_to_victims: dict):
    """pickOneNodeForPreemption, iterating the candidates in node-index order (every tie goes to the lowest index)"""
    if not nodes_to_victims:
        return None
    order = sorted(nodes_to_victims)
    for node in order:
        if len(nodes_to_victims[node]) == 0:
            return node
    min_nodes1 = order                                   # no PDBs: every node has 0 violations
    min_highest, min_nodes2 = MAX_INT32, []
    for node in min_nodes1:
        hp = nodes_to_victims[node][0]["priority"]
        if hp < min_highest:
            min_highest, min_nodes2 = hp, [node]
        elif hp == min_highest:
            min_nodes2.append(node)
    if len(min_nodes2) == 1:
        return min_nodes2[0]
    min_sum, min_nodes1 = MAX_INT64, []
    for node in min_nodes2:
        sp = sum(p["priority"] + (MAX_INT32 + 1) for p in nodes_to_victims[node])
        if sp < min_sum:
            min_sum, min_nodes1 = sp, [node]
        elif sp == min_sum:
            min_nodes1.append(node)
    if len(min_nodes1) == 1:
        return min_nodes1[0]
    min_num, min_nodes2 = MAX_INT32, []
    for node in min_nodes1:
        n = len(nodes_to_victims[node])
        if n < min_num:
            min_num, min_nodes2 = n, [node]
        elif n == min_num:
            min_nodes2.append(node)
    if len(min_nodes2) == 1:
        return min_nodes2[0]
    latest = earliest_start(nodes_to_victims[min_nodes2[0]])
    node_to_return = min_nodes2[0]
    for node in min_nodes2[1:]:
        e = earliest_start(nodes_to_victims[node])
        if e > latest:
            latest, node_to_return = e, node
    return node_to_return


def earliest_start(victims: list) -> int:
    """util.GetEarliestPodStartTime: the earliest start among the victims of the highest priority"""
    hp = max(p["priority"] for p in victims)
    return min(p["start"] for p in victims if p["priority"] == hp)


def preempt_obj(nodes, fit, pods, bound, S, pod_index, priority, protected, cap) -> dict:
    per = bound_objects(bound, S)
    fitb = fit.to_bool()
    q = len(pod_index)
    out = _empty(q, cap)
    for i, (pi, P) in enumerate(zip(pod_index, priority)):
        pi, P = int(pi), int(priority[i])
        req = [int(pods.req[j, pi]) for j in range(4 + S)]
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        nv = {}
        for k in range(nodes.n):
            if nodes.flags[k] or cls >= fitb.shape[0] or not fitb[cls, k]:
                continue
            victims, ok = select_victims_on_node(nodes, k, per.get(k, []), req, pres, grp, P, protected, S)
            if ok:
                nv[k] = victims
        out["n_candidates"][i] = len(nv)
        node = pick_one_node(nv)
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
            out["earliest_start"][i] = earliest_start(v)
    return out


def _empty(q: int, cap: int) -> dict:
    return dict(node=np.full(q, -1, np.int32), n_candidates=np.zeros(q, np.uint32), n_victims=np.zeros(q, np.uint32),
                victims=np.zeros((q, cap), np.uint32), top_priority=np.zeros(q, np.int32), priority_sum=np.zeros(q, np.int64),
                earliest_start=np.zeros(q, np.int64))


# ------------------------------------------------------------------------------------------------------------------------------
# numpy, vectorised over nodes
# ------------------------------------------------------------------------------------------------------------------------------
class Prep:
    """The bound table as padded [N, M] arrays in importance order per node (M = most pods on one node)."""

    def __init__(self, nodes, bound, S: int):
        N, L = nodes.n, 4 + S
        self.N, self.S, self.L = N, S, L
        node = bound.node.astype(np.int64)
        order = np.lexsort((np.arange(bound.b), bound.start_ns, -bound.priority.astype(np.int64), node))
        cnt = np.bincount(node, minlength=N) if bound.b else np.zeros(N, np.int64)
        M = max(int(cnt.max()) if N else 0, 1)
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if N else np.zeros(0, np.int64)
        sn = node[order]
        col = np.arange(bound.b) - start[sn] if bound.b else np.zeros(0, np.int64)
        self.M = M
        self.valid = np.zeros((N, M), bool)
        self.valid[sn, col] = True
        self.prio = np.full((N, M), 1 << 40, np.int64)           # padding: never below any preemptor's priority
        self.prio[sn, col] = bound.priority[order]
        self.start = np.zeros((N, M), np.int64)
        self.start[sn, col] = bound.start_ns[order]
        self.group = np.full((N, M), NOT_GROUPED, np.int64)
        self.group[sn, col] = bound.group[order]
        self.id = np.zeros((N, M), np.int64)
        self.id[sn, col] = order
        self.req = np.zeros((L, N, M), np.int64)                 # lane 3 = 1 pod; scalar lanes 0 where the key is absent
        for j in range(L):
            if j == 3:
                v = np.ones(bound.b, np.int64)
            elif j >= 4:
                v = np.where((bound.req_present >> np.uint32(j - 4)) & 1, bound.req[j], 0)
            else:
                v = bound.req[j]
            self.req[j][sn, col] = v[order]
        self.alloc = nodes.allocatable.astype(np.int64)
        self.apres = nodes.allocatable_present.astype(np.int64)
        cur = nodes.requested.astype(np.int64).copy()
        for s in range(S):
            cur[4 + s] = np.where((nodes.requested_present >> np.uint32(s)) & 1, cur[4 + s], 0)
        self.cur0 = cur                                          # [L, N] effective requests
        self.flags = nodes.flags


def holds_np(al, apres, cur, req, pres, S) -> np.ndarray:
    """holds() over node columns: al / cur [L, n], apres [n], req [L], pres int"""
    with np.errstate(over="ignore"):
        ok = np.ones(cur.shape[1], bool)
        for j in range(3):
            if req[j] > 0:
                ok &= ~(req[j] > al[j] - cur[j])
        ok &= ~(cur[3] + 1 > al[3])
        for s in range(S):
            if (pres >> s) & 1 and req[4 + s] > 0:
                ok &= ((apres >> s) & 1) != 0
                ok &= ~(req[4 + s] > al[4 + s] - cur[4 + s])
    return ok


def preempt_np(prep: Prep, fit, pods, pod_index, priority, protected, cap) -> dict:
    S, L, N = prep.S, prep.L, prep.N
    fitb = fit.to_bool() if N else np.zeros((0, 0), bool)
    prot = np.asarray(protected, bool) if protected is not None and len(protected) else np.zeros(1, bool)
    v_ung = prep.group == NOT_GROUPED
    v_bad = (prep.group == GROUP_MISSING) | ((prep.group >= 0) & prot[np.clip(prep.group, 0, None)])
    q = len(pod_index)
    out = _empty(q, cap)
    for i in range(q):
        pi, P = int(pod_index[i]), int(priority[i])
        req = pods.req[:L, pi].astype(np.int64)
        pres, cls, grp = int(pods.req_present[pi]), int(pods.cls[pi]), int(pods.group[pi])
        q_grouped = grp != NOT_GROUPED
        ok = prep.flags == 0
        ok &= fitb[cls] if cls < fitb.shape[0] else np.zeros(N, bool)
        vm = prep.valid & (prep.prio < P)                                      # potential victims [N, M]
        bad = np.where(v_ung, q_grouped, v_bad | (q_grouped & (prep.group == grp)))
        ok &= ~np.any(vm & bad, axis=1)
        with np.errstate(over="ignore"):
            cur = prep.cur0 - (prep.req * vm[None]).sum(axis=2)                # remove all
        ok &= holds_np(prep.alloc, prep.apres, cur, req, pres, S)
        cand = np.nonzero(ok)[0]
        out["n_candidates"][i] = cand.size
        if cand.size == 0:
            continue
        al, ap, c, m = prep.alloc[:, cand], prep.apres[cand], cur[:, cand], vm[cand]
        rq, pr, st, ids = prep.req[:, cand], prep.prio[cand], prep.start[cand], prep.id[cand]
        victim = np.zeros(m.shape, bool)
        with np.errstate(over="ignore"):
            for col in range(prep.M):
                mc = m[:, col]
                if not mc.any():
                    continue
                t = c + rq[:, :, col] * mc[None]
                h = holds_np(al, ap, t, req, pres, S)
                c = np.where((mc & h)[None], t, c)
                victim[:, col] = mc & ~h
        nv = victim.sum(axis=1)
        if np.any(nv == 0):
            w = int(np.nonzero(nv == 0)[0][0])
        else:
            first = victim.argmax(axis=1)                                      # first victim = highest priority, earliest start
            top = pr[np.arange(cand.size), first]
            est = st[np.arange(cand.size), first]
            ssum = np.where(victim, pr + (MAX_INT32 + 1), 0).sum(axis=1)
            w = int(np.lexsort((cand, ~est, nv, ssum, top))[0])        # ~est: the latest start first, no overflow
            out["top_priority"][i] = top[w]
            out["priority_sum"][i] = ssum[w]
            out["earliest_start"][i] = est[w]
        out["node"][i] = cand[w]
        out["n_victims"][i] = nv[w]
        vid = ids[w][victim[w]][:cap]
        out["victims"][i, : vid.size] = vid
    return out


def victims_of(res: dict, i: int) -> np.ndarray:
    return res["victims"][i, : min(int(res["n_victims"][i]), res["victims"].shape[1])]
