"""bs_wait_nodes_apply (include/bsched.h, "the wait table follows node-list surgery") as an array-level model on tests/wait_ref.Table
(TEST INFRASTRUCTURE).  Written from the header text, not from the HIP.

`nodes_apply` is the text taken literally: every row carries the CURRENT index of its node through the list; a REMOVE of index i drops the
rows that sit on i and moves the rows behind i down by one, an APPEND only raises the count, an UPDATE does nothing.  `by_identity` says the
same thing a second, independent way: an explicit Python list of node identities takes the deltas one at a time, and each row then looks its
node's identity up.  `device_rule` restates the device's arithmetic (csrc/bs_wait.hpp: the sorted removed list, one binary search per row,
the exclusive scan in blocks of 1024) so that the CPU tests can hold it against the model."""
import json
import os

import numpy as np

import wait_ref as wr

HERE = os.path.dirname(os.path.abspath(__file__))
UPDATE, APPEND, REMOVE = 0, 1, 2          # BS_DELTA_* (include/bsched.h)
BLOCK = 1024                              # kWtBlock


def _lists(kind, index):
    k, i = [int(x) for x in np.asarray(kind, np.int64).reshape(-1)], [int(x) for x in np.asarray(index, np.int64).reshape(-1)]
    assert len(k) == len(i)
    return k, i


def nodes_apply(tab, groups_matched, kind, index, n_expected=None, g=None):
    """bs_wait_nodes_apply on the model.  tab: wait_ref.Table (None: no table); groups_matched: the groups' matched column, changed in
    place; n_expected = bs_nodes_count (None: whatever the replay ends at); g = the loaded group count (None: the table's).  Returns
    dict(n, id, node, group): the dropped rows in ascending id with their OLD node.  On an error raises wait_ref.WaitError and changes nothing."""
    if tab is None:
        raise wr.WaitError(wr.STATE, "no table")
    if g is not None and tab.g != g:
        raise wr.WaitError(wr.STATE, "a stale group count")
    kl, il = _lists(kind, index)
    cur = tab.node.astype(np.int64).copy()                  # the row's node, by its index in the list as it is now
    alive = np.ones(tab.w, bool)
    count = tab.n
    for k, i in zip(kl, il):
        if k == APPEND:
            count += 1
        elif k == UPDATE or k == REMOVE:
            if not 0 <= i < count:
                raise wr.WaitError(wr.INVALID, f"index {i} at a count of {count}")
            if k == REMOVE:
                alive &= cur != i                           # (an appended node has no rows: nothing sits on it)
                cur[alive & (cur > i)] -= 1
                count -= 1
        else:
            raise wr.WaitError(wr.INVALID, f"kind {k}")
    if n_expected is not None and count != n_expected:
        raise wr.WaitError(wr.STATE, f"the replay ends at {count} nodes, the node list holds {n_expected}")
    gone = ~alive
    out = dict(n=int(gone.sum()), id=tab.id[gone].copy(), node=tab.node[gone].copy(), group=tab.group[gone].copy())
    for x in tab.group[gone]:
        groups_matched[int(x)] = np.uint32((int(groups_matched[int(x)]) - 1) & 0xFFFFFFFF)
    tab.node = cur.astype(np.uint32)
    tab._keep(alive)
    tab.n = count
    return out


def by_identity(n, node, kind, index):
    """the second statement, for a VALID list: -> (new node per row, -1 for a dropped row; the new count)"""
    nodes = [("old", k) for k in range(n)]
    serial = 0
    for k, i in zip(*_lists(kind, index)):
        if k == APPEND:
            nodes.append(("new", serial))
            serial += 1
        elif k == REMOVE:
            nodes.pop(i)
    where = {ident: pos for pos, ident in enumerate(nodes)}
    return np.array([where.get(("old", int(k)), -1) for k in np.asarray(node).reshape(-1)], np.int64), len(nodes)


def removed_sorted(n, kind, index):
    """the host half for a VALID list: the removed OLD nodes, ascending (what the device is handed), from the identities"""
    nodes = list(range(n))
    for k, i in zip(*_lists(kind, index)):
        if k == APPEND:
            nodes.append(-1)
        elif k == REMOVE:
            nodes.pop(i)
    return np.array(sorted(set(range(n)) - set(nodes)), np.int64)


def device_rule(tab, rem, cap=None):
    """csrc/bs_wait.hpp on a table: k_wn_map (lo = removed nodes below the row's node, by binary search; gone when the node is listed),
    k_wt_scan1 + k_wt_scan2 over the word survives << 32 | leaves in blocks of 1024, k_wn_move.
    Returns (columns of the new table, dropped rows (id, node, group) cut at cap, true count)."""
    rem = np.asarray(rem, np.int64)
    node = tab.node.astype(np.int64)
    lo = np.searchsorted(rem, node, side="left")
    gone = (lo < rem.size) & (rem[np.minimum(lo, max(rem.size - 1, 0))] == node) if rem.size else np.zeros(tab.w, bool)
    nnode = node - lo
    W = tab.w
    nblk = max(1, -(-W // BLOCK))
    word = np.zeros(nblk * BLOCK, np.uint64)
    word[:W] = np.where(gone, np.uint64(1), np.uint64(1) << np.uint64(32))
    blocks = word.reshape(nblk, BLOCK)
    inc = np.cumsum(blocks, axis=1, dtype=np.uint64)
    bsum = inc[:, -1]
    pre = np.concatenate([[np.uint64(0)], np.cumsum(bsum, dtype=np.uint64)[:-1]]).astype(np.uint64)
    pos = (inc - blocks + pre[:, None]).reshape(-1)[:W]
    total = int(pre[-1] + bsum[-1])
    kept, left = total >> 32, total & 0xFFFFFFFF
    new = dict(id=np.zeros(kept, np.uint32), node=np.zeros(kept, np.uint32), group=np.zeros(kept, np.int32), req=np.zeros((tab.L, kept), np.int64),
               req_present=np.zeros(kept, np.uint32))
    rows = dict(id=np.zeros(left, np.uint32), node=np.zeros(left, np.uint32), group=np.zeros(left, np.int32))
    for e in range(W):
        d, r = int(pos[e]) >> 32, int(pos[e]) & 0xFFFFFFFF
        if gone[e]:
            rows["id"][r], rows["node"][r], rows["group"][r] = tab.id[e], tab.node[e], tab.group[e]
        else:
            new["id"][d], new["node"][d], new["group"][d], new["req_present"][d] = tab.id[e], nnode[e], tab.group[e], tab.req_present[e]
            new["req"][:, d] = tab.req[:, e]
    k = left if cap is None else min(left, cap)
    return new, {f: v[:k] for f, v in rows.items()}, left


def remap_on_the_host(cols, n, kind, index):
    """the path the call replaces, for the twin contexts: bs_wait_read's columns -> (the columns to bs_wait_load, the dropped rows' groups)"""
    new, _ = by_identity(n, cols["node"], kind, index)
    keep = new >= 0
    return (new[keep].astype(np.uint32), cols["group"][keep], cols["req"][:, keep], cols["req_present"][keep]), cols["group"][~keep]


# ---- a real cycle under churn (tests/test_wait_nodes_cpu.py on the model, tests/test_gpu_wait_nodes.py on the device) ---------------------
def churn_scene(soa, S=1):
    """-> (nodes, fit, groups, pods1, pods2, steps).  Six nodes that hold 6 pods each; cycle 1 leaves 15 pods of three gangs waiting on
    nodes 0, 1 and 2 (first fit), nodes 3, 4, 5 stay empty.  steps: node 0 (holds rows) and nodes 3, 4, 5 (hold none) leave, four empty
    nodes are appended: the list becomes [old 1, old 2, new, new, new, new] (with fewer nodes the second pass rejects the gangs).  pods2 are the members that arrive for cycle 2: gang 2 gets the one it
    lacks, the others too few."""
    from test_gpu_seq_expire import waiting_scene
    nodes, fit, groups, pods1 = waiting_scene(soa, [5, 4, 6], n_nodes=6, S=S, pods_cap=6, matched0=[0, 1, 0], seed=77)
    rng = np.random.default_rng(78)
    group = np.array([0, 1, 2, 0, 1, 0, 1, 0], np.int32)
    P, L = group.size, 4 + S
    req = np.zeros((L, P), np.int64)
    req[0] = rng.integers(1, 20, P)
    req[1] = rng.integers(1, 1 << 20, P)
    pres = (rng.integers(0, 1 << S, P) if S else np.zeros(P, np.int64)).astype(np.uint32)
    req[4:] = rng.integers(1, 4, (S, P)) * ((pres[None, :] >> np.arange(S, dtype=np.uint32)[:, None]) & 1)
    pods2 = soa.Pods(group, req, pres, np.zeros(P, np.uint32), np.zeros(P, np.uint64), np.zeros(P, np.uint8))
    steps = [(REMOVE, 0), (APPEND, 1), (REMOVE, 2), (REMOVE, 2), (REMOVE, 2), (APPEND, 2), (APPEND, 3), (APPEND, 4)]      # old node 3 is index 2 once node 0 is gone
    return nodes, fit, groups, pods1, pods2, steps


def hand_kats():
    with open(os.path.join(HERE, "golden", "wait_nodes_hand_kats.json")) as f:
        return json.load(f)["scenes"]
