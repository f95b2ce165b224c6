"""Rule SP of include/bsched.h as a node choice for tests/seq_soa_ref.seq_pass (TEST INFRASTRUCTURE): the second statement of
bs_seq_run_scored_nominated, from arrays.  The candidates are built from work.E with rule S's test — the node's lanes plus every live row on
it with priority >= the pod's that is not the pod's own, every lane wrapping, a scalar lane counted where the row's bit is set —, the choice
among them is rule P's over the node's RAW lanes (D8: no row enters a score), and the pod's own row dies when the pod is assumed (D6).  The
object model tests/seq_scored_nominated_ref.py is the first statement; tests/test_seq_scored_nominated_cpu.py holds the two together."""
import numpy as np

import seq_scored_ref as ssr
from seq_soa_ref import NOM_NONE, w64


class ScoredNominatedChoice:
    """rows: the columns of bs_nominated_read (table order); priority [p], own_id [p] or None; weights (w_least, w_most, w_balanced).
    total [p] and n_fit [p] are what bs_seq_score_read returns, consumed what bs_seq_nominated_read returns (before sorting by id)."""

    def __init__(self, rows, priority, own_id, weights, p):
        m = 0 if rows is None else len(rows["id"])
        self.rows = [dict(id=int(rows["id"][x]), node=int(rows["node"][x]), priority=int(rows["priority"][x]), pres=int(rows["req_present"][x]),
                          req=[int(v) for v in rows["req"][:, x]]) for x in range(m)]
        self.priority, self.own_id = priority, own_id
        self.weights = tuple(int(v) for v in weights)
        self.total, self.n_fit = np.zeros(p, np.uint32), np.zeros(p, np.uint32)
        self.consumed = []

    def seen(self, work, k, P_i, own):
        """the lanes and key bits rule S's fit test of node k sees"""
        have, hpres = work.have(k), int(work.nodes.requested_present[k])
        for o in self.rows:
            if o["node"] != k or o["priority"] < P_i or o["id"] == own:
                continue
            for j in range(4):
                have[j] = w64(have[j] + o["req"][j])
            for s in range(work.S):
                if (o["pres"] >> s) & 1:
                    have[4 + s] = w64((have[4 + s] if (hpres >> s) & 1 else 0) + o["req"][4 + s])
                    hpres |= 1 << s
        return have, hpres

    def __call__(self, i, C, work):
        P_i = int(self.priority[i])
        own = NOM_NONE if self.own_id is None else int(self.own_id[i])
        cand = [k for k in work.E if work.holds(k, *self.seen(work, k, P_i, own))]       # (C, the table-less set, is not consulted)
        self.n_fit[i] = len(cand)
        if not cand:
            return -1
        nd = work.nodes
        tot = [ssr.total_of(int(nd.allocatable[0, k]), w64(int(nd.requested[0, k]) + work.r[0]),
                            int(nd.allocatable[1, k]), w64(int(nd.requested[1, k]) + work.r[1]), self.weights) for k in cand]
        top = max(tot)
        self.total[i] = top
        at = cand[tot.index(top)]
        if own != NOM_NONE:
            gone = [o for o in self.rows if o["id"] == own]
            assert len(gone) == 1, "an own id names one live row"
            self.rows.remove(gone[0])
            self.consumed.append((own, i, at))
        return at

    def live_ids(self):
        return np.array([o["id"] for o in self.rows], np.uint32)
