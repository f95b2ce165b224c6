"""The sequential pass once more, in plain Python over the SoA arrays, with the node choice as a parameter (TEST INFRASTRUCTURE).

`seq_pass` is the loop of oracle/bs_oracle_seq.c (orc_seq_replay) restated on Python ints: per pod the C oracle's own PreFilter
(`orc.Sop.prefilter`, on a Sop carried with the leader; its struct points at the working arrays, so the in-place writes below are what the
next PreFilter reads), the two `continue` rules, the candidate set C in list order (node flags, checkFit bit, holds), `at = choose(...)`,
the assume step, Permit and the release at the quorum.  PreFilter only.  Three choices:

  first_fit       C's first member: the pass of orc.seq_replay
  NominatedChoice rule S of include/bsched.h: the fit test of node k sees the requests plus every live row on k with priority >= the
                  pod's that is not the pod's own row, every lane added wrapping, a scalar lane counted where the row's bit is set; the
                  pod's own row dies when the pod is assumed on any node (D6)
  ScoredChoice    rule P: among C the largest seq_scored_ref.total_of, ties to the lowest index

This is the third statement of each rule (beside the object models tests/seq_nominated_ref.py and tests/seq_scored_ref.py, and the C
oracle for first fit), and the only one that starts from arrays: tests/world_ref.py runs it on a World's state.  tests/test_seq_soa_cpu.py
pins it against the other two."""
import numpy as np

import seq_scored_ref as ssr

M64 = (1 << 64) - 1
NOM_NONE = 0xFFFFFFFF
GROUP_SCHEDULED_LATCH, GROUP_PHASE_CLOSED = 0x01, 0x10      # BS_GROUP_* of include/bsched.h (tests/test_seq_soa_cpu.py holds them against soa's)


def w64(v: int) -> int:
    """int64 wrap-around"""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def holds(alloc, apres: int, have, hpres: int, r, pres: int, S: int, mutate=None) -> bool:
    """bs_oracle_seq.c, holds(): alloc / have are the node's allocatable and requested lanes as Python ints, apres / hpres their key bits
    (mutate: see MUTANTS)"""
    for j in range(3):
        if (r[j] > 0 or mutate == "zero_binds") and r[j] > w64(alloc[j] - have[j]):
            return False
    if have[3] + 1 > alloc[3] or (mutate == "pods_lane_lt" and have[3] + 1 == alloc[3]):
        return False
    for s in range(S):
        if not (pres >> s) & 1 or r[4 + s] <= 0:
            continue
        if not (apres >> s) & 1:
            return False
        rq = have[4 + s] if (hpres >> s) & 1 else 0
        if r[4 + s] > alloc[4 + s] - rq:
            return False
    return True


class Work:
    """what a choice sees of the pass: the working nodes (requests as the earlier pods left them) and the pod at hand"""

    def __init__(self, nodes, S):
        self.nodes, self.S, self.L = nodes, S, 4 + S
        self.E, self.r, self.pres = [], None, 0         # the eligible nodes of the pod at hand (flags, checkFit), its request, its key bits
        self.mutate = None

    def alloc(self, k):
        return [int(self.nodes.allocatable[j, k]) for j in range(self.L)]

    def have(self, k):
        return [int(self.nodes.requested[j, k]) for j in range(self.L)]

    def holds(self, k, have=None, hpres=None) -> bool:
        nd = self.nodes
        return holds(self.alloc(k), int(nd.allocatable_present[k]), self.have(k) if have is None else have,
                     int(nd.requested_present[k]) if hpres is None else hpres, self.r, self.pres, self.S, self.mutate)


def first_fit(i, C, work):
    return C[0] if C else -1


class NominatedChoice:
    """rule S over the rows of bs_nominated_read (a dict of columns, table order); priority [p], own_id [p] or None"""

    def __init__(self, rows, priority, own_id=None):
        m = 0 if rows is None else len(rows["id"])
        self.rows = [dict(id=int(rows["id"][x]), node=int(rows["node"][x]), priority=int(rows["priority"][x]), pres=int(rows["req_present"][x]),
                          req=[int(v) for v in rows["req"][:, x]]) for x in range(m)]
        self.by_node = {}
        for o in self.rows:
            self.by_node.setdefault(o["node"], []).append(o)
        self.priority, self.own_id = priority, own_id
        self.consumed, self.blocked = [], 0

    def seen(self, work, k, P_i, own):
        """the lanes and key bits the fit test of node k sees: the node's plus the qualifying rows'"""
        have, hpres = work.have(k), int(work.nodes.requested_present[k])
        mine = [o for o in self.by_node.get(k, ()) if o["priority"] >= P_i and o["id"] != own]
        for o in mine:
            for j in range(4):
                have[j] = w64(have[j] + o["req"][j])
            for s in range(work.S):
                if (o["pres"] >> s) & 1:
                    have[4 + s] = w64((have[4 + s] if (hpres >> s) & 1 else 0) + o["req"][4 + s])
                    hpres |= 1 << s
        return have, hpres, bool(mine)

    def __call__(self, i, C, work):
        P_i = int(self.priority[i])
        own = NOM_NONE if self.own_id is None else int(self.own_id[i])
        at, turned = -1, False
        for k in work.E:
            have, hpres, any_row = self.seen(work, k, P_i, own)
            if work.holds(k, have, hpres):
                at = k
                break
            turned |= any_row and k in C
        self.blocked += int(turned)
        if at >= 0 and own != NOM_NONE:
            gone = [o for o in self.rows if o["id"] == own]
            assert len(gone) == 1, "an own id names one live row"
            self.rows.remove(gone[0])
            self.by_node[gone[0]["node"]].remove(gone[0])
            self.consumed.append((own, i, at))
        return at

    def live_ids(self):
        return np.array([o["id"] for o in self.rows], np.uint32)


class ScoredChoice:
    """rule P; total [p] and n_fit [p] are what bs_seq_score_read returns"""

    def __init__(self, weights, p):
        self.weights = tuple(int(v) for v in weights)
        self.total, self.n_fit = np.zeros(p, np.uint32), np.zeros(p, np.uint32)

    def __call__(self, i, C, work):
        self.n_fit[i] = len(C)
        if not C:
            return -1
        nd = work.nodes
        tot = [ssr.total_of(int(nd.allocatable[0, k]), w64(int(nd.requested[0, k]) + work.r[0]),
                            int(nd.allocatable[1, k]), w64(int(nd.requested[1, k]) + work.r[1]), self.weights) for k in C]
        top = max(tot)
        self.total[i] = top
        return C[tot.index(top)]


# single-rule changes of the assume / Permit / release block below (tests/test_seq_hand_cpu.py: every one of them has to disagree with a
# hand-derived answer of tests/golden/seq_hand_kats.json).  seq_pass(..., mutate=None) is the pass itself.
MUTANTS = ("quorum_gt", "quorum_signed", "release_this_pass", "postbind_one", "close_gt", "closed_releases", "no_latch_closed", "matched_kept",
           "nonode_counted", "rollback_unreleased", "pods_lane_not_bumped", "pods_lane_lt", "zero_binds", "flags_ignored", "fitbit_ignored",
           "no_present_bit", "last_fit")


def seq_pass(orc, nodes, fit, groups, pods, leader, choose, mutate=None) -> dict:
    """-> what orc.seq_replay returns (without its timings), plus assumed [p] (the node every pod was assumed on, -1 none) and wait_node [p]
    as seq_expire_ref.waiting_after_pass states it.  Works on copies of nodes and groups.  mutate: one name of MUTANTS, the pass with that one
    rule changed (a wrong pass on purpose)."""
    assert mutate is None or mutate in MUTANTS, mutate
    nodes = nodes.copy()
    snap = orc.Snapshot(nodes, fit)
    sop = orc.Sop(snap, groups).carry(leader)
    gr = sop.groups
    S, N, G, P = nodes.lanes - 4, nodes.n, int(gr.g), pods.p
    L = 4 + S
    fitb = fit.to_bool()
    work = Work(nodes, S)
    work.mutate = mutate
    pf, fk, ld = np.zeros(P, np.uint8), np.zeros(P, np.uint32), np.zeros(P, np.int32)
    pod_node, assumed = np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    waiting = {}                                            # group -> the pods of this pass that wait at Permit
    rel_group, rel_pods, slot_of = [], [], {}
    open_nodes = [k for k in range(N) if not nodes.flags[k] or mutate == "flags_ignored"]
    for i in range(P):
        gi = int(pods.group[i])
        grouped = 0 <= gi < G
        pf[i], fk[i] = sop.prefilter(pods, i)
        ld[i] = sop.leader
        if pf[i] >= 16:
            continue
        if gi != -1 and not grouped:
            continue
        r = [int(pods.req[j, i]) for j in range(L)]
        pres, cls = int(pods.req_present[i]), int(pods.cls[i])
        work.r, work.pres = r, pres
        work.E = [k for k in open_nodes if (cls < fit.n_classes and fitb[cls, k]) or mutate == "fitbit_ignored"]
        C = [k for k in work.E if work.holds(k)]
        at = choose(i, C[::-1] if mutate == "last_fit" else C, work)
        if at < 0 and not (mutate == "nonode_counted" and grouped):
            continue
        for j in range(3 if at >= 0 else 0):
            nodes.requested[j, at] = w64(int(nodes.requested[j, at]) + r[j])
        if at >= 0 and mutate != "pods_lane_not_bumped":
            nodes.requested[3, at] = w64(int(nodes.requested[3, at]) + 1)
        for s in range(S if at >= 0 else 0):
            if (pres >> s) & 1:
                if not (int(nodes.requested_present[at]) >> s) & 1:
                    nodes.requested[4 + s, at] = 0
                nodes.requested[4 + s, at] = w64(int(nodes.requested[4 + s, at]) + r[4 + s])
                if mutate != "no_present_bit":
                    nodes.requested_present[at] |= np.uint32(1 << s)
        assumed[i] = at
        if not grouped:
            pod_node[i] = at
            continue
        gr.matched[gi] = (int(gr.matched[gi]) + 1) & 0xFFFFFFFF
        waiting.setdefault(gi, []).append(i)
        m1, mm, sc0 = int(gr.matched[gi]), int(gr.min_member[gi]), int(gr.status_scheduled[gi])
        if mutate == "quorum_gt":
            ready = m1 > ((mm - sc0) & 0xFFFFFFFF)
        elif mutate == "quorum_signed":
            ready = m1 >= mm - sc0
        else:
            ready = orc.permit_ready(m1, mm, sc0)
        if not ready:
            continue
        is_closed = bool(int(gr.flags[gi]) & GROUP_PHASE_CLOSED)
        if not (is_closed and mutate == "no_latch_closed"):
            gr.flags[gi] |= GROUP_SCHEDULED_LATCH
        if is_closed and mutate != "closed_releases":
            continue
        here = waiting.pop(gi)
        k = len(here) if mutate == "release_this_pass" else m1
        for w in here:
            pod_node[w] = assumed[w]
        if mutate != "matched_kept":
            gr.matched[gi] = 0
        gr.status_scheduled[gi] = (sc0 + (1 if mutate == "postbind_one" else k)) & 0xFFFFFFFF
        if int(gr.status_scheduled[gi]) >= mm + (1 if mutate == "close_gt" else 0):
            gr.flags[gi] |= GROUP_PHASE_CLOSED
        if gi in slot_of:
            rel_pods[slot_of[gi]] = (rel_pods[slot_of[gi]] + k) & 0xFFFFFFFF      # (a uint32 on the device and in the C oracle)
        else:
            slot_of[gi] = len(rel_group)
            rel_group.append(gi)
            rel_pods.append(k)
    if mutate == "rollback_unreleased":
        for i in (w for ws in waiting.values() for w in ws if assumed[w] >= 0):
            at = int(assumed[i])
            for j in range(3):
                nodes.requested[j, at] = w64(int(nodes.requested[j, at]) - int(pods.req[j, i]))
            nodes.requested[3, at] = w64(int(nodes.requested[3, at]) - 1)
            for s in range(S):
                if (int(pods.req_present[i]) >> s) & 1:
                    nodes.requested[4 + s, at] = w64(int(nodes.requested[4 + s, at]) - int(pods.req[4 + s, i]))
    grouped = (pods.group >= 0) & (pods.group < G)
    wait = np.where(grouped & (assumed >= 0) & (pod_node < 0), assumed, -1).astype(np.int32)
    return dict(pf_code=pf, pf_first_k=fk, pf_leader=ld, pod_node=pod_node, released_group=np.array(rel_group, np.uint32),
                released_pods=np.array(rel_pods, np.uint32), n_released=len(rel_group), nodes=nodes, groups=gr, leader=sop.leader,
                assumed=assumed, wait_node=wait)
