"""The resident Permit-wait table (bs_wait_*) as an array-level model (TEST INFRASTRUCTURE).

Written from the text of include/bsched.h ("the resident Permit-wait table"), not from the HIP: plain numpy and Python over
tests/seq_expire_ref.State (node requests + keys, group matched + flags, the last pass's waiting pods).  What the reference does:
MatchedPodNodes keeps one entry per waiting pod with a TTL of its own (core.go:284-309, :289-290); at the quorum every entry binds
(batchscheduler.go:292-333); when the gang's PodNameUIDs entry runs out every entry is rejected, its pod leaves its node, the entries are
deleted and the group goes onto the deny list (controller.go:322-332).  The clock stays with the caller."""
import numpy as np

import seq_expire_ref as ser

INVALID, STATE, CAPACITY = -1, -4, -5
WAIT_MAX = 1 << 24
DENIED = ser.DENIED


class WaitError(Exception):
    def __init__(self, status, why):
        super().__init__(f"{why}: status {status}")
        self.status = status


class Table:
    """rows in ascending id; n, g: the node count and group count the table was created for; S: the context's scalar lanes"""

    def __init__(self, n, g, S):
        self.n, self.g, self.S, self.L = n, g, S, 4 + S
        self.id, self.node, self.group = np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32)
        self.req, self.req_present = np.zeros((self.L, 0), np.int64), np.zeros(0, np.uint32)
        self.ids = 0

    @property
    def w(self):
        return int(self.id.size)

    def copy(self):
        t = Table(self.n, self.g, self.S)
        t.id, t.node, t.group, t.req, t.req_present, t.ids = self.id.copy(), self.node.copy(), self.group.copy(), self.req.copy(), self.req_present.copy(), self.ids
        return t

    def columns(self):
        return dict(id=self.id, node=self.node, group=self.group, req=self.req, req_present=self.req_present)

    def _append(self, ids, node, group, req, pres):
        self.id = np.concatenate([self.id, np.asarray(ids, np.uint32)])
        self.node = np.concatenate([self.node, np.asarray(node, np.uint32)])
        self.group = np.concatenate([self.group, np.asarray(group, np.int32)])
        self.req = np.concatenate([self.req, np.asarray(req, np.int64).reshape(self.L, -1)], axis=1)
        self.req_present = np.concatenate([self.req_present, np.asarray(pres, np.uint32)])

    def _keep(self, keep):
        self.id, self.node, self.group, self.req, self.req_present = self.id[keep], self.node[keep], self.group[keep], self.req[:, keep], self.req_present[keep]


def stored(req, pres, S):
    """request lanes as the assume step counted the pod: lanes 0..2 the request, the pods lane 1, a scalar lane the request where the present
    bit is set, else 0; the present bits masked to the scalar lanes"""
    req = np.array(req, np.int64).reshape(4 + S, -1).copy()
    pres = (np.asarray(pres, np.uint32).reshape(-1) & np.uint32((1 << S) - 1)).astype(np.uint32)
    req[3] = 1
    for s in range(S):
        req[4 + s] = np.where((pres >> s) & 1, req[4 + s], 0)
    return req, pres


def check(tab, n, g):
    """every call but load / count / ids: a table, created for the node count and group count the context holds now"""
    if tab is None:
        raise WaitError(STATE, "no table")
    if tab.n != n or tab.g != g:
        raise WaitError(STATE, "stale counts")


def load(n, g, S, node=(), group=(), req=None, req_present=None, w=None):
    """bs_wait_load -> a fresh Table.  Validated as a whole."""
    node, group = np.asarray(node, np.int64).reshape(-1), np.asarray(group, np.int64).reshape(-1)
    w = node.size if w is None else w
    if w > WAIT_MAX:
        raise WaitError(CAPACITY, "more than BS_WAIT_MAX entries")
    if np.any(node >= n) or np.any(group < 0) or np.any(group >= g):
        raise WaitError(INVALID, "a node or a group out of range")
    t = Table(n, g, S)
    if w:
        r, p = stored(np.zeros((4 + S, w), np.int64) if req is None else req, np.zeros(w, np.uint32) if req_present is None else req_present, S)
        t._append(np.arange(w), node, group, r, p)
    t.ids = w
    return t


def park(st, tab, pods):
    """bs_wait_park: every pod the last pass left waiting (st.wait_node >= 0) moves into the table, ascending queue index.  The caller has
    checked the window.  matched, flags and node requests do not change."""
    check(tab, st.requested.shape[1], st.matched.size)
    idx = np.nonzero(st.wait_node >= 0)[0]
    n = int(idx.size)
    if tab.ids + n > WAIT_MAX:
        raise WaitError(CAPACITY, "the id space would pass BS_WAIT_MAX")
    first = tab.ids
    out = dict(first_id=first, n=n, pod=idx.astype(np.uint32), node=st.wait_node[idx].astype(np.uint32))
    if n:
        r, p = stored(pods.req[:, idx], pods.req_present[idx], tab.S)
        tab._append(first + np.arange(n), st.wait_node[idx], pods.group[idx], r, p)
        tab.ids += n
        st.wait_node[idx] = -1
    return out


def _group_list(tab, groups):
    gl = [int(x) for x in np.asarray(groups, np.int64).reshape(-1)]
    if any(x < 0 or x >= tab.g for x in gl):
        raise WaitError(INVALID, "a group index out of range")
    if len(set(gl)) != len(gl):
        raise WaitError(INVALID, "a group listed twice")
    return gl


def _leave(st, tab, rows):
    """NodeInfo.RemovePod for table rows: lanes 0..2 minus the request, the pods lane minus 1, a scalar lane the row has a present bit for
    loses the request and keeps its node bit, other scalar lanes keep word and bit; a key the node lacks counts as 0 and its bit becomes
    set (RemovePod's map rule); wrapping int64"""
    for e in rows:
        k, pres = int(tab.node[e]), int(tab.req_present[e])
        for j in range(3):
            st.requested[j, k] = ser.w64(int(st.requested[j, k]) - int(tab.req[j, e]))
        st.requested[3, k] = ser.w64(int(st.requested[3, k]) - 1)
        for s in range(tab.S):
            if (pres >> s) & 1:
                if not (int(st.requested_present[k]) >> s) & 1:
                    st.requested[4 + s, k] = 0
                    st.requested_present[k] |= np.uint32(1 << s)
                st.requested[4 + s, k] = ser.w64(int(st.requested[4 + s, k]) - int(tab.req[4 + s, e]))


def release(tab, groups, n, g):
    """bs_wait_release: the rows of the listed groups leave the table by a stable compaction; nothing else changes"""
    check(tab, n, g)
    gl = _group_list(tab, groups)
    gone = np.isin(tab.group, gl)
    out = dict(n=int(gone.sum()), id=tab.id[gone].copy(), node=tab.node[gone].copy(),
               group_entries=np.array([int((tab.group == x).sum()) for x in gl], np.uint32))
    tab._keep(~gone)
    return out


def expire(st, tab, groups, deny=False, flags=None):
    """bs_wait_expire: the rows of the listed groups leave the table and their nodes; matched = 0 for every listed group; deny"""
    check(tab, st.requested.shape[1], st.matched.size)
    fl = (1 if deny else 0) if flags is None else flags
    if fl & ~1:
        raise WaitError(INVALID, "unknown flag bits")
    gl = _group_list(tab, groups)
    gone = np.isin(tab.group, gl)
    entries = np.array([int((tab.group == x).sum()) for x in gl], np.uint32)
    out = dict(n=int(gone.sum()), id=tab.id[gone].copy(), node=tab.node[gone].copy(), group_entries=entries,
               group_unknown=np.array([(int(st.matched[x]) - int(e)) & 0xFFFFFFFF for x, e in zip(gl, entries)], np.uint32))
    _leave(st, tab, np.nonzero(gone)[0])
    for x in gl:
        st.matched[x] = 0
        if fl & 1:
            st.flags[x] |= np.uint8(DENIED)
    tab._keep(~gone)
    return out


def forget(st, tab, ids):
    """bs_wait_forget: single rows by id — live and distinct —: each leaves the table and its node, matched of its group falls by 1 (uint32)"""
    check(tab, st.requested.shape[1], st.matched.size)
    il = [int(x) for x in np.asarray(ids, np.int64).reshape(-1)]
    if any(x < 0 or x >= tab.ids for x in il):
        raise WaitError(INVALID, "an unknown id")
    if len(set(il)) != len(il):
        raise WaitError(INVALID, "an id listed twice")
    where = {int(v): e for e, v in enumerate(tab.id)}
    if any(x not in where for x in il):
        raise WaitError(INVALID, "a dead id")
    rows = [where[x] for x in il]
    node_out = tab.node[rows].astype(np.uint32)
    _leave(st, tab, rows)
    for e in rows:
        gi = int(tab.group[e])
        st.matched[gi] = np.uint32((int(st.matched[gi]) - 1) & 0xFFFFFFFF)
    keep = np.ones(tab.w, bool)
    keep[rows] = False
    tab._keep(keep)
    return node_out


# ---- the two-cycle scenario (tests/test_wait_cpu.py on the model, tests/test_gpu_wait.py on the device) ---------------------------------
def two_cycle_scene(soa, seed, S=None):
    """-> (nodes, fit, groups, pods1, pods2, completes).  Cycle 1: no gang reaches its quorum, every placed pod waits.  The queue then
    loses every pod of cycle 1 that got a node (they are parked) and gains new members: gangs in `completes` get the members they lack
    and are released in cycle 2, the others get too few (some none) and stay short.  Pods of cycle 1 that found no node stay queued."""
    from test_gpu_seq_expire import waiting_scene
    rng = np.random.default_rng(seed)
    G = int(3 + seed % 4)
    S = int(seed % 3) if S is None else S
    lens = [int(x) for x in rng.integers(1, 6, G)]
    matched0 = [int(x) for x in rng.integers(0, 2, G)]
    nodes, fit, groups, pods1 = waiting_scene(soa, lens, n_nodes=int(2 + seed % 4), S=S, pods_cap=int(6 + seed % 5), interleave=bool(seed % 2), matched0=matched0,
                                              seed=seed + 1000)
    extra = rng.integers(0, 3, G)
    extra[int(rng.integers(0, G))] = 0
    extra[int(rng.integers(0, G))] = max(int(extra.max()), 1) if G > 1 else 0
    groups.min_member[:] = groups.min_member + extra.astype(groups.min_member.dtype)    # lacks 1 + extra members after cycle 1
    completes = [g for g in range(G) if extra[g] == 0]
    new_lens = [1 if extra[g] == 0 else int(rng.integers(0, extra[g] + 1)) for g in range(G)]
    L = 4 + S
    group = np.repeat(np.arange(G, dtype=np.int32), new_lens)
    P = group.size
    req = np.zeros((L, P), np.int64)
    req[0] = rng.integers(1, 20, P)
    req[1] = rng.integers(1, 1 << 20, P)
    pres = (rng.integers(0, 1 << S, P) if S else np.zeros(P, np.int64)).astype(np.uint32)
    req[4:] = rng.integers(1, 4, (S, P)) * ((pres[None, :] >> np.arange(S, dtype=np.uint32)[:, None]) & 1)
    pods2 = soa.Pods(group, req, pres, np.zeros(P, np.uint32), np.zeros(P, np.uint64), np.zeros(P, np.uint8))
    return nodes, fit, groups, pods1, pods2, completes


def second_queue(soa, pods1, parked, pods2):
    """the queue of cycle 2: cycle 1's pods without the parked ones (nobody was released in cycle 1), then the new members"""
    rest = pods1.take(np.setdiff1d(np.arange(pods1.p), np.asarray(parked, np.int64)))
    return soa.Pods(*[np.concatenate([getattr(rest, f), getattr(pods2, f)], axis=-1) for f in ("group", "req", "req_present", "cls", "owner", "flags")])
