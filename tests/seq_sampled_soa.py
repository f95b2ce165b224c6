"""Rule F of include/bsched.h as a node choice for tests/seq_soa_ref.seq_pass (TEST INFRASTRUCTURE): the second statement of the two
sampled passes, from arrays.  Where the object model (tests/seq_sampled_ref.py) sorts the candidates by visit position and cuts the list,
this one WALKS: v = 0 .. N - 1, node (s + v) mod N, a counter of members; the walk ends on the member that takes the counter past K, and V
is the v it ends on.  The candidates are rule P's (seq_pass's own C) or, composed with a seq_soa_ref.NominatedChoice, rule S's — that
object's `seen` gives the lanes the fit test sees, and its rows are where the pod's own row dies (D6).  The total is
seq_scored_ref.total_of over the node's raw lanes.  tests/test_seq_sampled_cpu.py holds the two statements together."""
import numpy as np

import seq_scored_ref as ssr
from seq_soa_ref import NOM_NONE, w64


class SampledChoice:
    """sample = (num_to_find, start); weights (w_least, w_most, w_balanced); p, n: the pods of the queue, the nodes of the list; nominated: a
    seq_soa_ref.NominatedChoice (rule SP underneath) or None (rule P).  total / n_fit are what bs_seq_score_read returns, start / visited / next_start what bs_seq_sample_read returns;
    consumed what bs_seq_nominated_read returns (before sorting by id)."""

    def __init__(self, sample, weights, p, n, nominated=None):
        self.num_to_find = int(sample[0])
        self.cursor = int(sample[1]) % n if n else 0            # what the next walk starts at; behind the pass: next_start
        self.weights = tuple(int(v) for v in weights)
        self.nom = nominated
        self.total, self.n_fit = np.zeros(p, np.uint32), np.zeros(p, np.uint32)
        self.start, self.visited = np.zeros(p, np.uint32), np.zeros(p, np.uint32)
        self.consumed = []

    @property
    def next_start(self):
        return self.cursor

    def member(self, i, k, C, E, work):
        """is node k in the candidate set of the form underneath?  C: rule P's set, E: the nodes the skip rule leaves (both as sets)"""
        if self.nom is None:
            return k in C
        if k not in E:
            return False
        own = NOM_NONE if self.nom.own_id is None else int(self.nom.own_id[i])
        have, hpres, _ = self.nom.seen(work, k, int(self.nom.priority[i]), own)
        return work.holds(k, have, hpres)

    def __call__(self, i, C, work):
        N = work.nodes.n
        K = N if self.num_to_find == 0 or self.num_to_find >= N else self.num_to_find
        s, C, E = self.cursor, set(C), set(work.E)
        found, best, at, V = 0, -1, -1, N
        nd = work.nodes
        for v in range(N):
            k = s + v
            if k >= N:
                k -= N
            if not self.member(i, k, C, E, work):
                continue
            if found == K:                                      # the (K+1)-th member: not kept, the walk ends in front of it
                V = v
                break
            found += 1
            t = ssr.total_of(int(nd.allocatable[0, k]), w64(int(nd.requested[0, k]) + work.r[0]),
                             int(nd.allocatable[1, k]), w64(int(nd.requested[1, k]) + work.r[1]), self.weights)
            if t > best:                                        # (strictly: an equal total later in the walk loses)
                best, at = t, k
        self.start[i], self.visited[i], self.n_fit[i] = s, V, found
        self.cursor = (s + V) % N if N else 0
        if at < 0:
            return -1
        self.total[i] = best
        if self.nom is not None:
            own = NOM_NONE if self.nom.own_id is None else int(self.nom.own_id[i])
            if own != NOM_NONE:
                gone = [o for o in self.nom.rows if o["id"] == own]
                assert len(gone) == 1, "an own id names one live row"
                self.nom.rows.remove(gone[0])
                self.nom.by_node[gone[0]["node"]].remove(gone[0])
                self.consumed.append((own, i, at))
        return at

    def live_ids(self):
        return self.nom.live_ids()
