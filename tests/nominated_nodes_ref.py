"""bs_nominated_nodes_apply (include/bsched.h, "the nominated-pod table follows node-list surgery") as an array-level model on
tests/nominated_ref.NomTable (TEST INFRASTRUCTURE).  Written from the header text, not from the HIP.  Built on nominated_ref.py and
bound_nodes_ref.py by import; neither is edited.

`nodes_apply` is the text taken literally: every row carries the CURRENT index of its node through the list; a REMOVE of index i drops the
rows that sit on i and moves the rows behind i down by one, an APPEND only raises the count, an UPDATE does nothing.  `by_identity` says the
same thing a second, independent way: an explicit Python list of node identities takes the deltas one at a time, with the rows as objects
that look their node's identity up.  `device_rule` restates the device's arithmetic (csrc/bs_nominated.hpp, k_nn_move: the sorted removed
list, one binary search per row, the stable compaction window by window with a running base, a dropped row at e - survivors before it) so
that the CPU tests can hold it against the model."""
import json
import os

import numpy as np

import nominated_ref as nr

HERE = os.path.dirname(os.path.abspath(__file__))
UPDATE, APPEND, REMOVE = 0, 1, 2          # BS_DELTA_* (include/bsched.h)
WINDOW = 1024                             # kNmWindow


def _lists(kind, index):
    k, i = [int(x) for x in np.asarray(kind, np.int64).reshape(-1)], [int(x) for x in np.asarray(index, np.int64).reshape(-1)]
    assert len(k) == len(i)
    return k, i


def nodes_apply(tab, kind, index, n_expected=None, single_rank=True):
    """bs_nominated_nodes_apply on the model.  tab: nominated_ref.NomTable (None or not loaded: no table); n_expected = bs_nodes_count
    (None: whatever the replay ends at).  Returns dict(n, id, node, priority): the dropped rows in ascending id with their OLD node.  On
    an error raises nominated_ref.NomRefused and changes nothing."""
    if not single_rank:
        raise nr.NomRefused("BS_ERR_STATE", "a sharded or external-reduce context")
    if tab is None or not tab.loaded:
        raise nr.NomRefused("BS_ERR_STATE", "no table")
    kl, il = _lists(kind, index)
    cur = tab.node.astype(np.int64).copy()                  # the row's node, by its index in the list as it is now
    alive = np.ones(tab.id.size, bool)
    count = tab.n
    for k, i in zip(kl, il):
        if k == APPEND:
            count += 1
        elif k == UPDATE or k == REMOVE:
            if not 0 <= i < count:
                raise nr.NomRefused("BS_ERR_INVALID", f"index {i} at a count of {count}")
            if k == REMOVE:
                alive &= cur != i                           # (an appended node has no rows: nothing sits on it)
                cur[alive & (cur > i)] -= 1
                count -= 1
        else:
            raise nr.NomRefused("BS_ERR_INVALID", f"kind {k}")
    if n_expected is not None and count != n_expected:
        raise nr.NomRefused("BS_ERR_STATE", f"the replay ends at {count} nodes, the node list holds {n_expected}")
    gone = ~alive
    out = dict(n=int(gone.sum()), id=tab.id[gone].copy(), node=tab.node[gone].copy(), priority=tab.prio[gone].copy())
    tab.id, tab.node, tab.prio, tab.pres, tab.req = tab.id[alive], cur[alive].astype(np.uint32), tab.prio[alive], tab.pres[alive], tab.req[:, alive]
    tab.n = count
    return out


def by_identity(n, rows: list, kind, index):
    """the second statement, for a VALID list.  rows: row objects (nominated_ref.rows_as_objects).  -> (surviving objects with their new
    node, dropped objects as they were, the new count)"""
    nodes = [("old", k) for k in range(n)]
    serial = 0
    for k, i in zip(*_lists(kind, index)):
        if k == APPEND:
            nodes.append(("new", serial))
            serial += 1
        elif k == REMOVE:
            nodes.pop(i)
    where = {ident: pos for pos, ident in enumerate(nodes)}
    kept, dropped = [], []
    for r in rows:
        if ("old", r["node"]) in where:
            kept.append(dict(r, node=where[("old", r["node"])]))
        else:
            dropped.append(dict(r))
    return kept, dropped, len(nodes)


def removed_sorted(n, kind, index):
    """the host half for a VALID list: the removed OLD nodes, ascending (what the device is handed), from the identities"""
    nodes = list(range(n))
    for k, i in zip(*_lists(kind, index)):
        if k == APPEND:
            nodes.append(-1)
        elif k == REMOVE:
            nodes.pop(i)
    return np.array(sorted(set(range(n)) - set(nodes)), np.int64)


def device_rule(rows: dict, rem, cap=None):
    """k_nn_move on the columns `rows` (NomTable.read()): lo = removed nodes below the row's node, by binary search; gone when the node is
    listed; windows of 1024 rows with a running base of survivors; a survivor to base + rank, a dropped row to e - survivors in front.
    Returns (columns of the new table, dropped rows (id, node, priority) cut at cap, true count)."""
    rem = np.asarray(rem, np.int64)
    node = rows["node"].astype(np.int64)
    W = node.size
    lo = np.searchsorted(rem, node, side="left")
    gone = (lo < rem.size) & (rem[np.minimum(lo, max(rem.size - 1, 0))] == node) if rem.size else np.zeros(W, bool)
    new = dict(id=np.zeros(W, np.uint32), node=np.zeros(W, np.uint32), priority=np.zeros(W, np.int32), req=np.zeros_like(rows["req"]),
               req_present=np.zeros(W, np.uint32))
    out = dict(id=np.zeros(W, np.uint32), node=np.zeros(W, np.uint32), priority=np.zeros(W, np.int32))
    base = 0
    for w0 in range(0, W, WINDOW):
        keep = ~gone[w0: w0 + WINDOW]
        rank = np.cumsum(keep) - keep                       # survivors in front of the row inside the window
        for t in range(keep.size):
            e, d = w0 + t, base + int(rank[t])
            if keep[t]:
                new["id"][d], new["node"][d], new["priority"][d], new["req_present"][d] = rows["id"][e], node[e] - lo[e], rows["priority"][e], rows["req_present"][e]
                new["req"][:, d] = rows["req"][:, e]
            else:
                out["id"][e - d], out["node"][e - d], out["priority"][e - d] = rows["id"][e], node[e], rows["priority"][e]
        base += int(keep.sum())
    left = W - base
    new = {f: (v[:, :base] if f == "req" else v[:base]) for f, v in new.items()}
    k = left if cap is None else min(left, cap)
    return new, {f: v[:k] for f, v in out.items()}, left


def remap_on_the_host(rows: dict, n, kind, index, S):
    """the path the call replaces, for the twin contexts: bs_nominated_read's columns -> the columns to bs_nominated_load"""
    kept, _, _ = by_identity(n, nr.rows_as_objects(rows, S), kind, index)
    return nr.objects_as_rows(kept, S)


def hand_kats():
    with open(os.path.join(HERE, "golden", "nominated_nodes_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_table(case) -> nr.NomTable:
    t = nr.NomTable(0)
    w = len(case["table"]["node"])
    req = np.zeros((4, w), np.int64)
    req[0] = 1 + np.arange(w)                               # (distinct lanes: a row that moved shows)
    t.load(case["n"], case["table"]["node"], case["table"]["priority"], req, np.zeros(w, np.uint32))
    return t
