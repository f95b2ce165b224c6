"""bs_bound_bind as an array-level model (TEST INFRASTRUCTURE), written from the header paragraph of include/bsched.h ("pods that leave
Permit enter the bound table on the device"), not from the HIP.  It composes the two existing models: an insert-only delta on
bound_apply_ref.Table, and a by-id removal on wait_ref's table that touches neither nodes nor groups.  Refusals are predicted from the
validity paragraph; on a refusal nothing has changed.

The pass's results arrive as two arrays over the queue: pod_node (bs_seq_run's result block, -1 = no node) and wait_node (what
bs_seq_waiting_read reports: the node of a pod that still waits in the pass's chains, else -1)."""
import importlib

import numpy as np

import bound_apply_ref as bar
import wait_ref as wr

bsa = importlib.import_module("batch-scheduler_amd")
soa = bsa.soa
INVALID, STATE, CAPACITY = -1, -4, -5
BOUND_MAX = 1 << 24


class BindError(Exception):
    def __init__(self, status, why):
        super().__init__(f"{why}: status {status}")
        self.status = status


def rows(wtab, wait_ids, pods, pod_node, pod_index, S):
    """the call's rows in its order as (node, group, req [L][n], req_present): wait rows as stored, queue pods by bs_wait_park's rule"""
    L = 4 + S
    wl = [int(x) for x in wait_ids]
    pl = [int(x) for x in pod_index]
    where = {int(v): e for e, v in enumerate(wtab.id)} if wtab is not None else {}
    we = [where[x] for x in wl]
    node = [int(wtab.node[e]) for e in we] + [int(pod_node[p]) for p in pl]
    group = [int(wtab.group[e]) for e in we] + [int(pods.group[p]) for p in pl]
    req = np.zeros((L, len(node)), np.int64)
    pres = np.zeros(len(node), np.uint32)
    if we:
        req[:, : len(we)] = wtab.req[:, we]
        pres[: len(we)] = wtab.req_present[we]
    if pl:
        r, p = wr.stored(pods.req[:, pl], pods.req_present[pl], S)
        req[:, len(we):] = r
        pres[len(we):] = p
    return np.array(node, np.uint32), np.array(group, np.int32), req, pres


def bind(btab, wtab, n, g, wait_ids=(), pod_index=(), priority=(), start_ns=(), pdb=None, pods=None, pod_node=None, wait_node=None, window=True,
         single_rank=True):
    """bs_bound_bind.  btab: bound_apply_ref.Table or None (before bs_bound_load); wtab: wait_ref.Table or None; n, g: the node and group
    counts the context holds now; window: a successful bs_seq_run's results are valid.  Returns dict(first_id, node); raises BindError
    with nothing changed."""
    wl = [int(x) for x in np.asarray(wait_ids, np.int64).reshape(-1)]
    pl = [int(x) for x in np.asarray(pod_index, np.int64).reshape(-1)]
    if not single_rank:
        raise BindError(STATE, "a sharded or external-reduce context")
    if btab is None:
        raise BindError(STATE, "before bs_bound_load")
    if btab.n != n:
        raise BindError(STATE, "the bound table's node count differs")
    if (wl and wait_ids is None) or (pl and pod_index is None) or ((wl or pl) and (priority is None or start_ns is None)):
        raise BindError(INVALID, "a NULL required array")
    if not wl and not pl:
        return dict(first_id=btab.ids, node=np.zeros(0, np.uint32))
    if wl and (wtab is None or wtab.n != n or wtab.g != g):
        raise BindError(STATE, "no wait table, or stale counts")
    if pl and not window:
        raise BindError(STATE, "no pass window")
    if wl:
        if any(x < 0 or x >= wtab.ids for x in wl):
            raise BindError(INVALID, "a wait id at or above bs_wait_ids")
        live = set(int(v) for v in wtab.id)
        if any(x not in live for x in wl):
            raise BindError(INVALID, "a dead wait id")
        if len(set(wl)) != len(wl):
            raise BindError(INVALID, "a wait id listed twice")
    if pl:
        P = int(pods.p)
        if any(x < 0 or x >= P for x in pl):
            raise BindError(INVALID, "a pod index at or above the queue length")
        if len(set(pl)) != len(pl):
            raise BindError(INVALID, "a pod index listed twice")
        if any(int(pod_node[p]) < 0 for p in pl):
            raise BindError(INVALID, "a pod without a node")
        if any(int(wait_node[p]) >= 0 for p in pl):
            raise BindError(INVALID, "a pod that still waits")
    cnt = len(wl) + len(pl)
    if btab.ids + cnt > BOUND_MAX:
        raise BindError(CAPACITY, "the id space would pass BS_BOUND_MAX")
    node, group, req, pres = rows(wtab, wl, pods, pod_node, pl, btab.S)
    ins = soa.Bound(node, np.asarray(priority, np.int32).reshape(-1), np.asarray(start_ns, np.int64).reshape(-1), group, req, pres)
    assert ins.priority.size == cnt and ins.start_ns.size == cnt
    try:
        first = btab.apply(None, ins, pdb)
    except bar.ApplyError as e:
        raise BindError(e.status, str(e))
    if wl:
        wtab._keep(~np.isin(wtab.id, np.array(wl, np.uint32)))
    return dict(first_id=first, node=node)


def make_bound(node, priority, start_ns, S, rng=None, group=None):
    """a bound table to load: 100 millicores each (rng: random requests and scalar keys), ungrouped unless group is given"""
    b = len(node)
    out = soa.Bound.empty(b, 4 + S)
    out.node[:] = node
    out.priority[:] = priority
    out.start_ns[:] = start_ns
    out.group[:] = -1 if group is None else group
    out.req[0] = 100 if rng is None else rng.integers(1, 1000, b)
    out.req[3] = 1
    if S and rng is not None:
        out.req_present[:] = rng.integers(0, 1 << S, b)
        out.req[4:] = rng.integers(1, 9, (S, b))
    return out


def max_group(old, group):
    """the largest group index the table is held to name after inserting `group`"""
    return max([int(old)] + [int(x) for x in group])
