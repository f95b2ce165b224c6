"""GPU tests of the resident PodDisruptionBudgets (bs_pdb_load / bs_pdb_members_append / bs_pdb_allowed_apply / bs_pdb_read).  Every
comparison is bit-exact against the by-id model of tests/pdb_resident_ref.py: bs_bound_dump's pdb column through bs_bound_read's ids,
bs_pdb_read's per-node counts and budgets, and a TWIN context that gets the model's bits through bs_bound_pdb_set and must answer
bs_preempt_run and bs_preempt_commit the same in every field and leave the same state (a wrong per-node count shows there as a one-pass
reprieve).  Shapes: node counts around the four nodes per workgroup and one wave, list lengths around the 64-entry step, member runs of
0 / 1 / 3 / 9 mixed within a wave, 0 / 1 / 70 PDBs, an empty table, 0 and 2 scalar lanes."""
import ctypes
import importlib

import numpy as np
import pytest

import bound_nodes_ref as bn
import pdb_resident_ref as pr
import preempt_pdb_ref as pp
from preempt_scenes import groups_for
from test_gpu_bound_apply import CAP, _compare, _scene, _take, _trim, _ungrouped_pool

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth, capi = bsa.soa, bsa.synth, bsa.capi
LENS = [0, 1, 63, 64, 65, 130]
INVALID, STATE, CAPACITY = -1, -4, -5


def _ctx(sc):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    return ctx


class Pair:
    """the context under test (a), its twin (b: the model's bits through bs_bound_pdb_set) and what the model expects of both"""

    def __init__(self, sc):
        self.sc, self.a, self.b = sc, _ctx(sc), _ctx(sc)
        self.m = None
        self.cur = np.zeros(sc["bound"].b, np.uint8)            # the bit every id carries now, dead ids included
        self.nl = bn.NodeList(sc["nodes"], sc["fit"])

    def close(self):
        self.a.close()
        self.b.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _recomputed(self):
        self.cur = self.m.bits(self.a.bound_ids())
        self.b.bound_pdb_set(self.cur)

    def load(self, allowed, off, member):
        self.a.pdb_load(allowed, off, member)
        self.m = pr.Model(allowed, off, member)
        self._recomputed()

    def allowed_apply(self, index, value):
        self.a.pdb_allowed_apply(index, value)
        if len(index):                                           # count == 0 launches nothing: the bits the table carries stay
            self.m.allowed_apply(index, value)
            self._recomputed()

    def members_append(self, off, member):
        self.a.pdb_members_append(self.m.covered, off, member)
        self.m.append(off, member)
        self._recomputed()

    def pdb_set(self, bits):
        """bs_bound_pdb_set on the context under test too: the last writer wins"""
        self.cur = np.asarray(bits, np.uint8).copy()
        self.a.bound_pdb_set(self.cur)
        self.b.bound_pdb_set(self.cur)

    def bound_apply_ex(self, rem, ins, pdb):
        first = self.a.bound_apply_ex(rem, ins, pdb)
        assert self.b.bound_apply_ex(rem, ins, pdb) == first
        if ins is not None:
            self.cur = np.concatenate([self.cur, np.zeros(ins.b, np.uint8) if pdb is None else (np.asarray(pdb) != 0).astype(np.uint8)])

    def surgery(self, steps):
        """[(APPEND, like) | (REMOVE, index)]: bs_nodes_apply and bs_bound_nodes_apply on both contexts"""
        deltas = [self.nl.append(int(i)) if k == bn.APPEND else self.nl.remove(int(i)) for k, i in steps]
        for ctx in (self.a, self.b):
            ctx.apply_node_deltas(deltas)
            ctx.bound_nodes_apply([d.kind for d in deltas], [d.index for d in deltas])

    def commit(self, where, apply=True):
        sc = self.sc
        ra = self.a.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=CAP, apply=apply)
        rb = self.b.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=CAP, apply=apply)
        _compare(ra, rb, f"{where}: bs_preempt_commit vs the twin")
        return ra

    def check(self, where, run=True):
        a, b = self.a, self.b
        ids, nodes = a.read_bound()
        n = self.nl.n
        col, nviol = pr.columns(self.cur, ids, nodes, n)
        got = a.bound_dump()["pdb"]
        assert np.array_equal(got, col), f"{where}: pdb column differs at table positions {np.nonzero(got != col)[0][:8]} (ids {ids[np.nonzero(got != col)[0][:8]]})"
        if self.m is not None:
            rd = a.pdb_read()
            assert rd["n_pdb"] == self.m.n_pdb and rd["covered"] == self.m.covered, f"{where}: {rd['n_pdb']} PDBs, {rd['covered']} covered"
            assert np.array_equal(rd["allowed"], self.m.allowed), f"{where}: allowed"
            assert np.array_equal(rd["node_violating"], nviol), f"{where}: per-node counts differ at nodes {np.nonzero(rd['node_violating'] != nviol)[0][:8]}"
        # the twin: same table, same bits, same answers
        ids_b, nodes_b = b.read_bound()
        assert np.array_equal(ids, ids_b) and np.array_equal(nodes, nodes_b), f"{where}: the twin's table"
        da, db = a.bound_dump(), b.bound_dump()
        for f in da:
            assert np.array_equal(da[f], db[f]), f"{where}: column {f} vs the twin"
        ra, rb = a.read_node_requests(), b.read_node_requests()
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), f"{where}: node requests vs the twin"
        if run:
            sc = self.sc
            ga = a.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=CAP)
            gb = b.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=CAP)
            _compare(ga, gb, f"{where}: bs_preempt_run vs the twin")
            return ga
        return None


def _shape(S, n):
    if n == 1:
        counts = [130]
    elif n <= 5:
        counts = {3: [130, 0, 65], 4: [64, 1, 63, 0], 5: [65, 130, 0, 1, 64]}[n]
    elif n <= 65:
        counts = [LENS[(k * 5 + k // 6) % 6] for k in range(n)]
    else:
        return _scene(8300 + 3 * n + S, n, (0, 9), S, groups=0)[0]
    sc = _trim(_scene(730 + n + S, n, 130, S, groups=0)[0], counts)
    assert np.bincount(sc["bound"].node, minlength=n).tolist() == counts
    return sc


def _flip(rng, m, want_exhausted: bool, count=1):
    """`count` distinct indices whose budgets are, or are not, exhausted now, and new values on the other side of zero"""
    ex = m.allowed <= 0
    pick = np.nonzero(ex != want_exhausted)[0]
    idx = rng.permutation(pick if pick.size else np.arange(m.n_pdb))[:count]
    val = rng.choice(np.array([0, -1, pr.I32_MIN] if want_exhausted else [1, 7, pr.I32_MAX], np.int64), idx.size)
    return idx.astype(np.uint32), val.astype(np.int32)


def _deciding_pdb(m, cur):
    """a PDB with budget left that selects a pod whose bit is clear: exhausting it sets that bit.  None when there is none."""
    pod = np.repeat(np.arange(m.covered), np.diff(m.off.astype(np.int64)))
    cand = np.unique(m.member[cur[pod] == 0])
    return int(cand[0]) if cand.size else None


@pytest.mark.parametrize("S,n,n_pdb", [(0, 1, 70), (2, 3, 1), (0, 4, 0), (2, 5, 70), (0, 64, 70), (2, 65, 1), (0, 257, 70)])
def test_the_sequence_step_by_step(S, n, n_pdb):
    sc = _shape(S, n)
    rng = np.random.default_rng(31 * n + S)
    pool = _ungrouped_pool(60 + n + S, n, 6, S)
    ids0 = sc["bound"].b
    with Pair(sc) as p:
        where = f"S={S} n={n} n_pdb={n_pdb}"
        p.check(f"{where} before the load", run=False)
        # 1. load
        off, member = pr.random_members(rng, ids0, n_pdb)
        p.load(pr.random_allowed(rng, n_pdb), off, member)
        first = p.check(f"{where} 1 load")
        if n_pdb == 70:
            assert p.cur.any() and not p.cur.all() and (n > 65 or first["n_pdb_violations"].any()), "the bits change nothing: the comparison shows nothing"
        # 2. a budget flipped to exhausted and back
        if n_pdb:
            before = p.cur.copy()
            decides = _deciding_pdb(p.m, p.cur)
            idx, val = _flip(rng, p.m, True)
            if decides is not None:
                idx[0] = decides
            old = p.m.allowed[idx].copy()
            p.allowed_apply(idx, val)
            p.check(f"{where} 2 exhausted")
            assert (p.cur >= before).all() and (decides is None or (p.cur != before).any())
            p.allowed_apply(idx, old)
            p.check(f"{where} 2 and back")
            assert np.array_equal(p.cur, before)
        # 3. removes and inserts: positions shift; the inserted ids are uncovered
        live, _ = p.a.read_bound()
        rem = rng.permutation(live)[: max(1, live.size // 6)]
        c = n + 7
        ins = _take(pool, rng.integers(0, pool.b, c), rng.integers(0, n, c))
        p.bound_apply_ex(rem, ins, np.ones(c, np.uint8))
        p.check(f"{where} 3 bs_bound_apply_ex")                         # (no recompute yet: the inserted entries carry pdb_violating)
        p.allowed_apply([], [])                                         # count == 0: nothing launched, the carried bits stay
        p.check(f"{where} 3 an empty apply", run=False)
        assert p.cur[ids0:].all()
        if n_pdb:
            idx, val = _flip(rng, p.m, False)
            p.allowed_apply(idx, val)
            assert not p.cur[ids0:].any(), "an uncovered id has no PDB"
            p.check(f"{where} 3 the next recompute")
        # 4. now covered
        off2, member2 = pr.random_members(rng, c, n_pdb, sizes=(1, 3, 9))
        p.members_append(off2, member2)
        p.check(f"{where} 4 bs_pdb_members_append")
        assert p.m.covered == ids0 + c and (n_pdb != 70 or p.cur[ids0:].any())
        # 5. compaction, dead ids
        res = p.commit(f"{where} 5")
        p.check(f"{where} 5 bs_preempt_commit(APPLY)")
        print(f"{where}: {int(first['n_victims'].sum())} victims of bs_preempt_run after the load, {int(first['n_pdb_violations'].sum())} violating; "
              f"{int(res['n_victims'].sum())} evicted by the commit")
        # 6.
        if n_pdb:
            idx, val = _flip(rng, p.m, True, 3)
            p.allowed_apply(idx, val)
            p.check(f"{where} 6 bs_pdb_allowed_apply")
        # 7. node-list surgery
        p.surgery([(bn.REMOVE, n // 2), (bn.APPEND, 0)] if n > 1 else [(bn.APPEND, 0), (bn.REMOVE, 0)])
        p.check(f"{where} 7 bs_bound_nodes_apply")
        # 8.
        if n_pdb:
            idx, val = _flip(rng, p.m, False, 2)
            p.allowed_apply(idx, val)
        else:
            p.members_append([0], [])                                   # n == 0: a recompute and nothing else
        p.check(f"{where} 8 bs_pdb_allowed_apply")


def test_an_empty_table_and_down_to_one():
    sc = _scene(77, 5, (1, 3), 2, groups=0)[0]
    b = sc["bound"]
    none = np.zeros(0, np.int64)
    sc["bound"] = soa.Bound(b.node[none], b.priority[none], b.start_ns[none], b.group[none], b.req[:, none], b.req_present[none])
    pool = _ungrouped_pool(78, 5, 4, 2)
    with Pair(sc) as p:
        p.load([0, 3], [0], [])
        p.check("an empty table")
        assert p.a.pdb_read()["node_violating"].tolist() == [0] * 5
        p.allowed_apply([1], [0])
        p.check("an empty table, a budget patched")
        p.bound_apply_ex([], _take(pool, [0, 1, 2], [4, 0, 4]), [1, 0, 1])
        p.members_append([0, 1, 1, 3], [0, 1, 0])
        p.check("three entries, covered")
        assert p.cur.tolist() == [1, 0, 1]
        p.allowed_apply([0, 1], [1, 1])
        p.check("nobody exhausted")
        assert not p.cur.any()
        p.bound_apply_ex([0, 1, 2], None, None)
        p.allowed_apply([0], [0])
        p.check("down to an empty table")
        assert p.a.bound_count() == 0 and p.a.pdb_read()["covered"] == 3


def test_fuzz_two_hundred_steps():
    S, n, n_pdb = 2, 6, 5
    sc = _scene(4242, n, (0, 8), S, q=6, groups=0)[0]
    pool = _ungrouped_pool(4243, n, 6, S)
    rng = np.random.default_rng(4244)
    kinds = dict(apply=0, apply_ex=0, append=0, commit=0, surgery=0, pdb_set=0, reload=0)
    with Pair(sc) as p:
        off, member = pr.random_members(rng, sc["bound"].b, n_pdb)
        p.load(pr.random_allowed(rng, n_pdb), off, member)
        for step in range(220):
            u = rng.random()
            ids = p.a.bound_ids()
            if u < 0.4:
                kind = "apply"
                idx = rng.permutation(n_pdb)[: int(rng.integers(1, n_pdb + 1))]
                p.allowed_apply(idx, pr.random_allowed(rng, idx.size, 0.4))
            elif u < 0.6:
                kind = "apply_ex"
                live, _ = p.a.read_bound()
                c = int(rng.integers(0, 9))
                p.bound_apply_ex(rng.permutation(live)[: int(rng.integers(0, min(live.size, 5) + 1))],
                                 _take(pool, rng.integers(0, pool.b, c), rng.integers(0, p.nl.n, c)) if c else None, rng.integers(0, 2, c) if c else None)
            elif u < 0.75:
                kind = "append"
                c = int(rng.integers(0, ids - p.m.covered + 1))                 # some of the uncovered ids, all of them, or none
                p.members_append(*pr.random_members(rng, c, n_pdb))
            elif u < 0.81:
                kind = "commit"
                p.commit(f"fuzz step {step}", apply=bool(rng.integers(0, 2)))
            elif u < 0.87:
                kind = "surgery"
                k = int(rng.integers(0, p.nl.n))
                p.surgery([(bn.REMOVE, k), (bn.APPEND, int(rng.integers(0, n)))] if rng.random() < 0.7 else [(bn.APPEND, 0)] if p.nl.n < 9 else [(bn.REMOVE, k)])
            elif u < 0.93:
                kind = "pdb_set"
                p.pdb_set(rng.integers(0, 2, ids).astype(np.uint8))
            else:
                kind = "reload"
                n_pdb = int(rng.integers(1, 9))
                off, member = pr.random_members(rng, ids, n_pdb)
                p.load(pr.random_allowed(rng, n_pdb), off, member)
            kinds[kind] += 1
            p.check(f"fuzz step {step} ({kind})", run=step % 8 == 0)
    assert all(v >= 3 for v in kinds.values()), kinds


def _snapshot(p):
    ids, nodes = p.a.read_bound()
    return dict(p.a.bound_dump(), id=ids, node=nodes, ids=np.array([p.a.bound_ids()]), **{"pdb_" + k: np.asarray(v) for k, v in p.a.pdb_read().items()})


def _refused(call, status, name):
    with pytest.raises(bsa.BsError) as e:
        call()
    assert e.value.status == status, f"{name}: status {e.value.status}, expected {status}"


def test_errors_leave_everything_unchanged():
    S, n, n_pdb = 2, 9, 6
    sc = _scene(901, n, (2, 9), S, groups=0)[0]
    pool = _ungrouped_pool(902, n, 4, S)
    rng = np.random.default_rng(903)
    B = sc["bound"].b
    off, member = pr.random_members(rng, B, n_pdb, sizes=(0, 1, 3))
    allowed = pr.random_allowed(rng, n_pdb, 0.5)
    u32, i32 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32)
    with bsa.Context(scalar_lanes=S, device=0) as ctx:                          # before bs_bound_load
        ctx.load_nodes(sc["nodes"], sc["fit"])
        for name, call in (("load", lambda: ctx.pdb_load(allowed, off, member)), ("append", lambda: ctx.pdb_members_append(0, [0], [])),
                           ("apply", lambda: ctx.pdb_allowed_apply([0], [0])), ("read", ctx.pdb_read)):
            _refused(call, STATE, name + " before bs_bound_load")
    with Pair(sc) as p:
        a = p.a
        for name, call in (("append", lambda: a.pdb_members_append(0, [0], [])), ("apply", lambda: a.pdb_allowed_apply([0], [0])),
                           ("an empty apply", lambda: a.pdb_allowed_apply([], [])), ("read", a.pdb_read)):
            _refused(call, STATE, name + " without bs_pdb_load")
        p.check("before any load", run=False)
        p.load(allowed, off, member)
        p.bound_apply_ex([3], _take(pool, [0, 1, 2, 3], [0, 1, 1, 8]), None)    # four uncovered ids; id 3 is dead
        p.check("the state the refused calls find")
        before = _snapshot(p)
        ids = B + 4
        lib, h = a._lib, a._h
        ptr = lambda v, t: np.ascontiguousarray(v).ctypes.data_as(t)            # noqa: E731
        keep = [np.asarray(allowed, np.int32), np.asarray(off, np.uint32), np.asarray(member, np.uint32)]
        long_off, _ = pr.random_members(rng, ids, n_pdb)
        bad_first = long_off.copy(); bad_first[0] = 1
        descending = long_off.copy(); descending[ids // 2] = descending[-1] + 1
        bad_member = np.zeros(int(long_off[-1]), np.uint32); bad_member[-1] = n_pdb
        huge = np.zeros(ids + 1, np.uint32); huge[1:] = (1 << 28) + 1
        ok_member = np.zeros(max(int(long_off[-1]), 1), np.uint32)
        many = np.zeros((1 << 20) + 1, np.int32)
        run_off = np.array([0, 1, 2], np.uint32)
        cases = [
            ("load: b != bs_bound_ids", INVALID, lambda: a.pdb_load(allowed, off, member)),                        # the load's B, now B + 4
            ("load: b above bs_bound_ids", INVALID, lambda: a.pdb_load(allowed, np.concatenate([long_off, long_off[-1:]]), ok_member)),
            ("load: offsets not from 0", INVALID, lambda: a.pdb_load(allowed, bad_first, ok_member)),
            ("load: offsets descend", INVALID, lambda: a.pdb_load(allowed, descending, np.zeros(int(descending.max()), np.uint32))),
            ("load: a member >= n_pdb", INVALID, lambda: a.pdb_load(allowed, long_off, bad_member)),
            ("load: more than BS_PDB_MEMBERS_MAX entries", CAPACITY, lambda: a.pdb_load(allowed, huge, ok_member)),
            ("load: more than BS_PDB_MAX PDBs", CAPACITY, lambda: a.pdb_load(many, long_off, ok_member)),
            ("append: first_id below covered", INVALID, lambda: a.pdb_members_append(B - 1, run_off, [0, 0])),
            ("append: first_id above covered", INVALID, lambda: a.pdb_members_append(B + 1, run_off, [0, 0])),
            ("append: first_id + n > ids", INVALID, lambda: a.pdb_members_append(B, [0, 1, 1, 1, 1, 2], [0, 0])),
            ("append: offsets not from 0", INVALID, lambda: a.pdb_members_append(B, [1, 1, 2], [0, 0])),
            ("append: offsets descend", INVALID, lambda: a.pdb_members_append(B, [0, 2, 1], [0, 0])),
            ("append: a member >= n_pdb", INVALID, lambda: a.pdb_members_append(B, run_off, [0, n_pdb])),
            ("append: more than BS_PDB_MEMBERS_MAX entries", CAPACITY, lambda: a.pdb_members_append(B, [0, 1 << 28], [0])),
            ("apply: an index >= n_pdb", INVALID, lambda: a.pdb_allowed_apply([0, n_pdb], [0, 0])),
            ("apply: an index listed twice", INVALID, lambda: a.pdb_allowed_apply([2, 1, 2], [0, 0, 0])),
            ("apply: more pairs than PDBs", INVALID, lambda: a.pdb_allowed_apply(np.arange(n_pdb + 1), np.zeros(n_pdb + 1))),
        ]
        for name, status, call in cases:
            _refused(call, status, name)
            after = _snapshot(p)
            for f in before:
                assert np.array_equal(before[f], after[f]), f"{name}: {f} changed"
        null = [("load: allowed NULL", lambda: lib.bs_pdb_load(h, n_pdb, None, ids, ptr(long_off, u32), ptr(ok_member, u32))),
                ("load: member_off NULL", lambda: lib.bs_pdb_load(h, n_pdb, ptr(keep[0], i32), ids, None, ptr(ok_member, u32))),
                ("load: member NULL", lambda: lib.bs_pdb_load(h, n_pdb, ptr(keep[0], i32), ids, ptr(long_off, u32), None)),
                ("append: member_off NULL", lambda: lib.bs_pdb_members_append(h, B, 2, None, ptr(ok_member, u32))),
                ("append: member NULL", lambda: lib.bs_pdb_members_append(h, B, 2, ptr(run_off, u32), None)),
                ("apply: index NULL", lambda: lib.bs_pdb_allowed_apply(h, 1, None, ptr(keep[0], i32))),
                ("apply: value NULL", lambda: lib.bs_pdb_allowed_apply(h, 1, ptr(run_off, u32), None))]
        assert long_off[-1] > 0
        for name, call in null:
            assert call() == INVALID, name
            after = _snapshot(p)
            for f in before:
                assert np.array_equal(before[f], after[f]), f"{name}: {f} changed"
        a.set_shard(0, 2)
        for name, call in (("load", lambda: a.pdb_load(allowed, long_off, ok_member)), ("append", lambda: a.pdb_members_append(B, run_off, [0, 0])),
                           ("apply", lambda: a.pdb_allowed_apply([0], [0]))):
            _refused(call, STATE, name + " on a sharded context")
        assert lib.bs_pdb_read(h, None, None, None, None) == STATE
        a.set_shard(0, 1)
        p.check("after the refused calls")                                      # the twin comparison, unchanged
        after = _snapshot(p)
        for f in before:
            assert np.array_equal(before[f], after[f]), f"after the refused calls: {f} changed"
        p.members_append(run_off, [0, n_pdb - 1])                               # and the context still works
        p.allowed_apply([n_pdb - 1, 0], [0, 1])
        p.check("after the refused calls, patched")


def test_bound_load_drops_the_state_and_pdb_set_wins_until_the_next_recompute():
    S, n, n_pdb = 0, 7, 4
    sc = _scene(311, n, (3, 12), S, groups=0)[0]
    rng = np.random.default_rng(312)
    B = sc["bound"].b
    off, member = pr.random_members(rng, B, n_pdb, sizes=(1, 3))
    with Pair(sc) as p:
        p.load([0, 1, 0, 5], off, member)
        p.check("loaded")
        assert p.cur.any()
        direct = rng.integers(0, 2, B).astype(np.uint8)
        assert not np.array_equal(direct, p.cur)
        p.pdb_set(direct)                                                       # bs_bound_pdb_set after a recompute: its bits stand
        p.check("bs_bound_pdb_set after a recompute")
        assert np.array_equal(p.a.pdb_read()["allowed"], [0, 1, 0, 5])          # (the resident state is untouched)
        p.pdb_set(np.zeros(B, np.uint8))
        p.check("bits cleared directly")
        p.allowed_apply([3], [4])                                               # the next recompute: the model's bits again
        p.check("the next recompute")
        assert p.cur.any()
        for ctx in (p.a, p.b):
            ctx.load_bound(sc["bound"])                                         # drops the state, clears the bits
        p.cur = np.zeros(B, np.uint8)
        p.m = None
        p.check("after bs_bound_load")
        for name, call in (("append", lambda: p.a.pdb_members_append(B, [0], [])), ("apply", lambda: p.a.pdb_allowed_apply([0], [0])), ("read", p.a.pdb_read)):
            _refused(call, STATE, name + " after bs_bound_load")
        p.load([1, 1, 1, 0], off, member)
        p.check("loaded again")


def test_relation_at_cfg3_size():
    """cfg3's node count, about 30 pods a node, 64 PDBs, 8 budgets flipped: the pdb column and the counts equal the model"""
    cfg = synth.CONFIGS["cfg3"]
    S, n, n_pdb = cfg["scalars"], cfg["nodes"], 64
    bound, nodes = synth.make_bound(20261018, n, 0, (20, 40), S)
    rng = np.random.default_rng(20261018)
    off, member = pr.random_members(rng, bound.b, n_pdb, sizes=(0, 1, 1, 2, 3))
    m = pr.Model(pr.random_allowed(rng, n_pdb, 0.1), off, member)
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, synth.make_fit(1, n, 4))
        ctx.load_bound(bound)
        ctx.pdb_load(m.allowed, off, member)
        ids, where = ctx.read_bound()
        for step in range(2):
            col, nviol = pr.columns(m.bits(bound.b), ids, where, n)
            rd = ctx.pdb_read()
            assert np.array_equal(ctx.bound_dump()["pdb"], col), f"step {step}: pdb column"
            assert np.array_equal(rd["node_violating"], nviol) and np.array_equal(rd["allowed"], m.allowed), f"step {step}: counts"
            assert 0 < col.sum() < col.size
            idx = rng.permutation(n_pdb)[:8]
            val = np.where(m.allowed[idx] <= 0, 3, 0)
            ctx.pdb_allowed_apply(idx, val)
            m.allowed_apply(idx, val)
        col, nviol = pr.columns(m.bits(bound.b), ids, where, n)
        assert np.array_equal(ctx.bound_dump()["pdb"], col) and np.array_equal(ctx.pdb_read()["node_violating"], nviol), "after the second flip"
