"""Two CPU restatements of the node half of bs_bound_apply_ex with BS_BOUND_NODES (include/bsched.h): the node requests follow a
bound-table delta, NodeInfo.RemovePod per removed entry and AddPod per inserted one.  The table half is tests/bound_apply_ref.py's model,
used as it is.

  State     numpy: per node the removed entries' stored columns are subtracted and the inserted ones added in one go (wrapping int64), a
            scalar lane none of them has keeps its word and its present bit.
  ObjState  object level: one NodeInfo per node with a dict of scalar keys; remove_pod / add_pod are called one entry at a time in the
            delta's order (removes first), and the dicts are written back.  It counts the additions that wrapped.

`scene(seed)` draws the seeded scenes both are held against each other on; `hand_kats()` reads the hand-typed known answers."""
from __future__ import annotations

import importlib
import json
import os

import numpy as np

import bound_apply_ref as ba

bsa = importlib.import_module("batch-scheduler_amd")
soa = bsa.soa
HERE = os.path.dirname(os.path.abspath(__file__))
BOUND_NODES = 1
MIN64, MAX64 = -(1 << 63), (1 << 63) - 1


def _wrap(x: int) -> int:
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


# ------------------------------------------------------------------------------------------------------------------------------
# numpy
# ------------------------------------------------------------------------------------------------------------------------------
class State:
    """the resident bound table (ba.Table) and the node requests (req [L, n], pres [n]) under bs_bound_apply_ex"""

    def __init__(self, bound, S: int, n: int, req, pres, bits=None):
        self.S, self.n = S, n
        self.t = ba.Table(bound, S, n, bits)
        self.req = np.array(req, np.int64, copy=True).reshape(4 + S, n)
        self.pres = np.array(pres, np.uint32, copy=True).reshape(n)

    def apply_ex(self, remove=None, insert=None, pdb=None, flags: int = BOUND_NODES) -> int:
        """raises ba.ApplyError and changes nothing on an error (an unknown flag bit among them)"""
        if flags & ~BOUND_NODES:
            raise ba.ApplyError(-1, "unknown flags")
        t = self.t
        old_id, old_node, old_req, old_pres = t.id, t.node, t.req, t.req_present     # (the model replaces its arrays, it never writes into them)
        first = t.apply(remove, insert, pdb)
        if not flags & BOUND_NODES:
            return first
        S, n, L = self.S, self.n, 4 + self.S
        rem = np.asarray([] if remove is None else remove, np.uint32).reshape(-1)
        sorter = np.argsort(old_id, kind="stable")
        pos = sorter[np.searchsorted(old_id, rem, sorter=sorter)] if rem.size else np.zeros(0, np.int64)
        d = np.zeros((L, n), np.int64)                   # inserts minus removes
        bits = np.zeros(n, np.uint32)
        hit = np.zeros(n, bool)
        with np.errstate(over="ignore"):
            for l in range(L):
                np.subtract.at(d[l], old_node[pos], old_req[l, pos])
            np.bitwise_or.at(bits, old_node[pos], old_pres[pos])
            hit[old_node[pos]] = True
            if insert is not None and insert.b:
                ireq, ipres = ba.stored(insert, S)
                for l in range(L):
                    np.add.at(d[l], insert.node, ireq[l])
                np.bitwise_or.at(bits, insert.node, ipres)
                hit[insert.node] = True
            bits &= np.uint32((1 << S) - 1)
            for l in range(L):
                if l < 4:
                    on, base = hit, self.req[l]
                else:
                    on = hit & (((bits >> np.uint32(l - 4)) & 1) != 0)
                    base = np.where((self.pres >> np.uint32(l - 4)) & 1, self.req[l], 0)
                self.req[l] = np.where(on, base + d[l], self.req[l])
        self.pres |= np.where(hit, bits, 0).astype(np.uint32)
        return first


# ------------------------------------------------------------------------------------------------------------------------------
# object level
# ------------------------------------------------------------------------------------------------------------------------------
class NodeInfo:
    """NodeInfo.requestedResource: milli-CPU, memory, ephemeral storage, the pod count and the ScalarResources map (present keys only)"""

    def __init__(self, cpu: int, mem: int, eph: int, pods: int, scalar: dict):
        self.cpu, self.mem, self.eph, self.pods, self.scalar = cpu, mem, eph, pods, dict(scalar)
        self.wraps = 0

    def _add(self, a: int, b: int) -> int:
        v = _wrap(a + b)
        self.wraps += v != a + b
        return v

    def add_pod(self, pod: dict):
        self.cpu, self.mem, self.eph = self._add(self.cpu, pod["cpu"]), self._add(self.mem, pod["mem"]), self._add(self.eph, pod["eph"])
        self.pods = self._add(self.pods, 1)
        for key, v in pod["scalar"].items():
            self.scalar[key] = self._add(self.scalar.get(key, 0), v)

    def remove_pod(self, pod: dict):
        self.cpu, self.mem, self.eph = self._add(self.cpu, -pod["cpu"]), self._add(self.mem, -pod["mem"]), self._add(self.eph, -pod["eph"])
        self.pods = self._add(self.pods, -1)
        for key, v in pod["scalar"].items():
            self.scalar[key] = self._add(self.scalar.get(key, 0), -v)


def _pods(bound, S: int) -> list:
    """the entries as pod objects: a scalar key is in the map where the entry's present bit (below S) is set"""
    return [dict(node=int(bound.node[i]), cpu=int(bound.req[0, i]), mem=int(bound.req[1, i]), eph=int(bound.req[2, i]),
                 scalar={s: int(bound.req[4 + s, i]) for s in range(S) if (int(bound.req_present[i]) >> s) & 1}) for i in range(bound.b)]


class ObjState:
    def __init__(self, bound, S: int, n: int, req, pres):
        self.S, self.n = S, n
        self.req = np.array(req, np.int64, copy=True).reshape(4 + S, n)
        self.pres = np.array(pres, np.uint32, copy=True).reshape(n)
        self.live = dict(enumerate(_pods(bound, S)))
        self.ids = bound.b
        self.wraps = 0

    def apply_ex(self, remove=None, insert=None, flags: int = BOUND_NODES) -> int:
        """a VALID delta (the numpy model refuses the others first)"""
        first = self.ids
        gone = [self.live.pop(int(i)) for i in ([] if remove is None else remove)]
        new = [] if insert is None else _pods(insert, self.S)
        for i, pod in enumerate(new):
            self.live[first + i] = pod
        self.ids += len(new)
        if not flags & BOUND_NODES:
            return first
        infos = {}
        for pod, leaving in [(p, True) for p in gone] + [(p, False) for p in new]:
            k = pod["node"]
            if k not in infos:
                infos[k] = NodeInfo(*(int(self.req[j, k]) for j in range(4)),
                                    {s: int(self.req[4 + s, k]) for s in range(self.S) if (int(self.pres[k]) >> s) & 1})
            (infos[k].remove_pod if leaving else infos[k].add_pod)(pod)
        for k, ni in infos.items():                       # write back: the four lanes, and every key the map holds (it is present now)
            self.req[0, k], self.req[1, k], self.req[2, k], self.req[3, k] = ni.cpu, ni.mem, ni.eph, ni.pods
            for s, v in ni.scalar.items():
                self.req[4 + s, k] = v
                self.pres[k] |= np.uint32(1 << s)
            self.wraps += ni.wraps
        return first


# ------------------------------------------------------------------------------------------------------------------------------
# scenes
# ------------------------------------------------------------------------------------------------------------------------------
KINDS = ("random", "absent_on_node", "remove_only_key", "wrap_and_return", "whole_node", "inserts_only")


def _values(rng, count, big: bool):
    v = rng.integers(0, 64, count).astype(np.int64) * 100
    if big:
        v = np.where(rng.random(count) < 0.5, rng.integers(1 << 61, MAX64, count, dtype=np.int64), v)
    return v


def _entries(rng, nodes, S: int, big: bool = False, pres=None):
    nodes = np.asarray(nodes, np.uint32).reshape(-1)
    b = nodes.size
    out = soa.Bound.empty(b, 4 + S)
    out.node[:] = nodes
    out.priority[:] = rng.integers(0, 4, b) * 100
    out.start_ns[:] = rng.integers(0, 3, b)
    for l in range(4 + S):
        out.req[l] = _values(rng, b, big)
    out.req[3] = rng.integers(0, 5, b)                    # whatever the caller says: the table stores 1
    out.req_present[:] = rng.integers(0, 1 << (S + 1), b) if pres is None else pres      # (a bit beyond S among them: masked)
    return out


def scene(seed: int) -> dict:
    """dict(kind, S, n, bound, req, pres, steps=[(remove ids, insert Bound or None)]), steps valid in sequence.  The kind (seed modulo
    the kinds) says which case the scene is built around; the random deltas around it run into the others too."""
    rng = np.random.default_rng(9000 + seed)
    kind = KINDS[seed % len(KINDS)]
    S = int(rng.choice([0, 1, 2, 4, 12])) if kind == "random" else int(rng.choice([1, 2, 4, 12]))
    n = int(rng.integers(1, 9))
    L = 4 + S
    big = kind == "wrap_and_return" or seed % 5 == 0
    counts = rng.integers(0, 7, n)
    if kind == "whole_node":
        counts[0] = max(counts[0], 2)
    if kind == "inserts_only":
        counts[n - 1] = 0
    bound = _entries(rng, np.repeat(np.arange(n), counts), S, big)
    req = np.stack([_values(rng, n, big) for _ in range(L)])
    pres = rng.integers(0, 1 << S, n).astype(np.uint32)
    if kind == "absent_on_node":
        pres[:] = 0                                        # the words stay: an absent key's word is no value
    if kind == "wrap_and_return":
        req[0, 0], req[1, 0] = MAX64 - 5, MIN64 + 5
    node_of = {i: int(bound.node[i]) for i in range(bound.b)}
    live = list(range(bound.b))
    ids = bound.b
    steps = []
    for step in range(int(rng.integers(2, 6))):
        rem, ins = [], None
        if step == 0 and kind == "whole_node":
            rem = [i for i in live if node_of[i] == 0]
        elif step == 0 and kind == "inserts_only":
            ins = _entries(rng, np.full(int(rng.integers(1, 4)), n - 1), S, big)
        elif step == 0 and kind == "remove_only_key":
            pool = [i for i in live if int(bound.req_present[i]) & ((1 << S) - 1)]
            rem = pool[:1] or live[:1]
        elif step == 0 and kind == "absent_on_node":
            ins = _entries(rng, rng.integers(0, n, 3), S, big, pres=(1 << S) - 1)
        elif step == 0 and kind == "wrap_and_return":    # lane 0 up past the maximum, lane 1 down past the minimum; step 1 takes both back
            ins = _entries(rng, [0, 0], S, False, pres=0)
            ins.req[0], ins.req[1] = [10, 20], [-10, -20]
        elif step == 1 and kind == "wrap_and_return":
            rem = [ids - 2, ids - 1]
        else:
            k = int(rng.integers(0, min(len(live), 5) + 1))
            rem = [int(i) for i in rng.permutation(live)[:k]]
            m = int(rng.integers(0, 5))
            ins = _entries(rng, rng.integers(0, n, m), S, big) if m else None
        for i in rem:
            live.remove(i)
        if ins is not None:
            for i in range(ins.b):
                node_of[ids + i] = int(ins.node[i])
                live.append(ids + i)
            ids += ins.b
        steps.append((rem, ins))
    return dict(kind=kind, S=S, n=n, bound=bound, req=req, pres=pres, steps=steps)


def hand_kats():
    with open(os.path.join(HERE, "golden", "bound_apply_nodes_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_entries(cols: dict, S: int):
    """a KAT's {node, req [L][b], req_present} as a Bound (priority 0, start = position, ungrouped)"""
    b = len(cols["node"])
    out = soa.Bound.empty(b, 4 + S)
    if b:
        out.node[:] = cols["node"]
        out.start_ns[:] = np.arange(b)
        out.req[:] = np.array(cols["req"], np.int64).reshape(4 + S, b)
        out.req_present[:] = cols["req_present"]
    return out
