"""Numpy model of the resident PodDisruptionBudgets (include/bsched.h, bs_pdb_load / bs_pdb_members_append / bs_pdb_allowed_apply), by
bound-pod id: the bit of id i is 1 iff i < covered and some m in member[member_off[i] .. member_off[i + 1]) has allowed[m] <= 0 as a
signed int32; an id at or beyond covered has bit 0.  Also the seeded scenes of string records tests/test_pdb_resident_cpu.py holds the
model against batch-scheduler_amd/pdb.py's violating_bits on, and random memberships for the GPU tests."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
BUDGETS = (0, 1, -1, I32_MIN, I32_MAX, 2, 7)


def bits_by_id(member_off, member, allowed, ids: int) -> np.ndarray:
    """uint8 [ids]: the rule above; covered = len(member_off) - 1"""
    off = np.asarray(member_off, np.int64).reshape(-1)
    mem = np.asarray(member, np.int64).reshape(-1)
    covered = max(off.size - 1, 0)
    assert covered <= ids
    out = np.zeros(ids, np.uint8)
    if covered:
        exhausted = np.asarray(allowed, np.int32).reshape(-1) <= 0
        run = np.concatenate([[0], np.cumsum(exhausted[mem])]) if mem.size else np.zeros(1, np.int64)
        out[:covered] = (run[off[1:]] - run[off[:-1]]) > 0
    return out


class Model:
    """the resident state under the three calls"""

    def __init__(self, allowed, member_off, member):
        self.allowed = np.array(allowed, np.int32).reshape(-1)
        self.off = np.array(member_off, np.uint32).reshape(-1) if len(member_off) else np.zeros(1, np.uint32)
        self.member = np.array(member, np.uint32).reshape(-1)
        assert self.off[0] == 0 and self.off[-1] == self.member.size

    @property
    def n_pdb(self) -> int:
        return int(self.allowed.size)

    @property
    def covered(self) -> int:
        return int(self.off.size - 1)

    def append(self, member_off, member):
        off = np.asarray(member_off, np.uint32).reshape(-1)
        if off.size > 1:
            self.off = np.concatenate([self.off, self.off[-1] + off[1:]]).astype(np.uint32)
            self.member = np.concatenate([self.member, np.asarray(member, np.uint32).reshape(-1)])

    def allowed_apply(self, index, value):
        self.allowed[np.asarray(index, np.int64)] = np.asarray(value, np.int32)

    def bits(self, ids: int) -> np.ndarray:
        return bits_by_id(self.off, self.member, self.allowed, ids)


def columns(bits, table_ids, table_nodes, n: int):
    """(pdb column in table order, per-node violating counts) of a live table whose entries have these ids and nodes"""
    col = np.asarray(bits, np.uint8)[np.asarray(table_ids, np.int64)] if len(table_ids) else np.zeros(0, np.uint8)
    return col, np.bincount(np.asarray(table_nodes, np.int64), weights=col, minlength=n).astype(np.uint32)[:n]


def random_members(rng, ids: int, n_pdb: int, sizes=(0, 1, 3, 9)):
    """(member_off, member) for `ids` ids: run lengths drawn from `sizes`, so lanes of one wave walk runs of different lengths"""
    ln = rng.choice(np.asarray(sizes), ids) if n_pdb and ids else np.zeros(ids, np.int64)
    off = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint32)
    return off, rng.integers(0, max(n_pdb, 1), int(off[-1])).astype(np.uint32)


def random_allowed(rng, n_pdb: int, exhausted: float = 0.3) -> np.ndarray:
    """budgets with the int32 edges among them; about `exhausted` of them are <= 0"""
    pos, neg = np.array([1, 2, 7, I32_MAX], np.int64), np.array([0, -1, I32_MIN], np.int64)
    return np.where(rng.random(n_pdb) < exhausted, rng.choice(neg, n_pdb), rng.choice(pos, n_pdb)).astype(np.int32)


# ---- scenes of string records (batch-scheduler_amd/pdb.py's dicts)
NAMESPACES = ("default", "kube-system", "")
KEYS = ("app", "tier", "zone", "track")
VALUES = ("a", "b", "c")
BROKEN = ({"matchExpressions": [{"key": "app", "operator": "Near", "values": ["a"]}]},          # unknown operator
          {"matchExpressions": [{"key": "app", "operator": "In", "values": []}]},               # In needs values
          {"matchExpressions": [{"key": "app", "operator": "Exists", "values": ["a"]}]},        # Exists takes none
          {"matchExpressions": [{"key": "not a key", "operator": "Exists"}]},
          {"matchLabels": {"app": "not a value!"}})
EMPTY = (None, {}, {"matchLabels": {}, "matchExpressions": []})


def _selector(rng):
    u = rng.random()
    if u < 0.12:
        return BROKEN[int(rng.integers(0, len(BROKEN)))]
    if u < 0.24:
        return EMPTY[int(rng.integers(0, len(EMPTY)))]
    sel = {}
    if rng.random() < 0.6:
        sel["matchLabels"] = {KEYS[int(k)]: VALUES[int(rng.integers(0, 3))] for k in rng.choice(4, int(rng.integers(1, 3)), replace=False)}
    exprs = []
    for _ in range(int(rng.integers(0 if sel else 1, 3))):
        op = ("In", "NotIn", "Exists", "DoesNotExist")[int(rng.integers(0, 4))]
        e = {"key": KEYS[int(rng.integers(0, 4))], "operator": op}
        if op in ("In", "NotIn"):
            e["values"] = [VALUES[int(v)] for v in rng.choice(3, int(rng.integers(1, 3)), replace=False)]
        exprs.append(e)
    if exprs:
        sel["matchExpressions"] = exprs
    return sel


def string_scene(seed: int):
    """(pdbs, bound_pods): namespaces, the four operators, unparsable / nil / empty selectors, label-less pods, budgets at the edges"""
    rng = np.random.default_rng(seed)
    pdbs = [{"namespace": NAMESPACES[int(rng.integers(0, 3))], "selector": _selector(rng), "disruptions_allowed": int(rng.choice(BUDGETS))}
            for _ in range(int(rng.integers(0, 9)))]
    pods = []
    for _ in range(int(rng.integers(0, 40))):
        u = rng.random()
        labels = None if u < 0.1 else {} if u < 0.2 else {KEYS[int(k)]: VALUES[int(rng.integers(0, 3))]
                                                           for k in rng.choice(4, int(rng.integers(1, 4)), replace=False)}
        pods.append({"namespace": NAMESPACES[int(rng.integers(0, 3))], "labels": labels})
    return pdbs, pods


def hand_kats():
    with open(os.path.join(HERE, "golden", "pdb_resident_hand_kats.json")) as f:
        return json.load(f)["scenes"]
