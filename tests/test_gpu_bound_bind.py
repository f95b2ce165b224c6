"""GPU tests of bs_bound_bind (csrc/bs_bound_bind.hpp) against the array model of tests/bound_bind_ref.py, bit for bit.  After every call:
bs_bound_read + bs_bound_dump, bs_bound_count / _ids, bs_wait_read / _count / _ids, and bs_nodes_read, bs_groups_read and (while the pass's
window is open) bs_seq_waiting_read, all three unchanged by the call.  Shapes are the smallest at which each kernel can go wrong: the rank
loop's 64-slot windows, the scans' blocks of 1024, the 256-thread kernels, BS_BOUND_MAX_PER_NODE."""
import ctypes as C

import numpy as np
import pytest

import bound_apply_ref as bar
import bound_bind_ref as bbr
import seq_expire_ref as ser
import wait_ref as wr
from test_gpu_bound_apply import _check_table
from test_gpu_parity import load_ctx
from test_gpu_seq import assert_groups_equal
from test_gpu_seq_expire import Case, status_of, waiting_scene, _node_delta
from test_gpu_wait import W

pytestmark = pytest.mark.gpu
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


class B:
    """a context with a bound table and (maybe) a wait table and a pass's results, and the models: bt, tab, and a snapshot of everything
    the call must not touch"""

    def __init__(self, ctx, soa, bt, tab, N, G, pods=None, pod_node=None, wait_node=None, window=False):
        self.ctx, self.soa, self.bt, self.tab, self.N, self.G = ctx, soa, bt, tab, N, G
        self.pods, self.pod_node, self.wait_node, self.window = pods, pod_node, wait_node, window
        self.rebase()

    def rebase(self):
        self.base = (self.ctx.read_node_requests(), self.ctx.read_groups(), self.ctx.seq_waiting_read() if self.window else None)

    def check(self, where):
        if self.bt is not None:
            _check_table(self.ctx, self.bt, where)
        if self.tab is not None:
            assert (self.ctx.wait_count(), self.ctx.wait_ids()) == (self.tab.w, self.tab.ids), f"{where}: wait count, ids"
            got = self.ctx.wait_read()
            for k, v in self.tab.columns().items():
                assert np.array_equal(got[k], v), f"{where}: wait table column {k}"
        (req, pres), groups, waiting = self.base
        r2, p2 = self.ctx.read_node_requests()
        assert np.array_equal(r2, req) and np.array_equal(p2, pres), f"{where}: node requests changed"
        assert_groups_equal(self.ctx.read_groups(), groups, self.soa, f"{where}: groups changed")
        if self.window:
            assert np.array_equal(self.ctx.seq_waiting_read(), waiting), f"{where}: bs_seq_waiting_read changed"
            if self.wait_node is not None:
                assert np.array_equal(waiting, self.wait_node), f"{where}: bs_seq_waiting_read vs the model"

    def bind(self, where, wl=(), pl=(), prio=None, start=None, pdb=None):
        n = len(wl) + len(pl)
        prio = np.zeros(n, np.int32) if prio is None else prio
        start = np.zeros(n, np.int64) if start is None else start
        exp = bbr.bind(self.bt, self.tab, self.N, self.G, wl, pl, prio, start, pdb, self.pods, self.pod_node, self.wait_node, window=self.window)
        got = self.ctx.bound_bind(wl, pl, prio, start, pdb)
        assert got["first_id"] == exp["first_id"], f"{where}: first_id {got['first_id']} vs {exp['first_id']}"
        assert np.array_equal(got["node"], exp["node"]), f"{where}: node_out"
        self.check(where)
        return got

    def refused(self, bsa, where, want, wl=(), pl=(), prio=None, start=None, pdb=None, model=True):
        n = len(wl) + len(pl)
        prio = np.zeros(n, np.int32) if prio is None else prio
        start = np.zeros(n, np.int64) if start is None else start
        if model:
            with pytest.raises(bbr.BindError) as e:
                bbr.bind(self.bt, self.tab, self.N, self.G, wl, pl, prio, start, pdb, self.pods, self.pod_node, self.wait_node, window=self.window)
            assert e.value.status == want, f"{where}: the model says {e.value.status}"
        assert status_of(bsa, lambda: self.ctx.bound_bind(wl, pl, prio, start, pdb)) == want, where
        self.check(f"{where}: refused, nothing changed")


def rows_ctx(bsa, soa, n_nodes, S, w_node, w_group, bound, G=2, rng=None, req=None, pres=None, bits=None):
    """a context with n_nodes nodes, G groups, a loaded bound table and a loaded wait table of the given rows (no pass)"""
    nodes, fit, groups, pods = waiting_scene(soa, [1] * G, n_nodes=n_nodes, S=S, seed=5)
    ctx = load_ctx(bsa, nodes, fit, groups, pods)
    w = len(w_node)
    L = 4 + S
    if req is None:
        req = np.zeros((L, w), np.int64) if rng is None else rng.integers(-9, 1 << 50, (L, w))
        pres = np.zeros(w, np.uint32) if rng is None else rng.integers(0, 1 << 13, w).astype(np.uint32)
    ctx.wait_load(w_node, w_group, req, pres)
    tab = wr.load(n_nodes, G, S, w_node, w_group, req, pres)
    bt = None
    if bound is not None:
        ctx.load_bound(bound)
        if bits is not None:
            ctx.bound_pdb_set(bits)
        bt = bar.Table(bound, S, n_nodes, bits=bits)
    return B(ctx, soa, bt, tab, n_nodes, G, pods=pods)


def released_case(bsa, soa, orc, lens, complete, **kw):
    """a pass over gangs of lens[g] pods; the gangs in `complete` reach their quorum and are released (placed, not waiting), the others wait"""
    nodes, fit, groups, pods = waiting_scene(soa, lens, **kw)
    for g in complete:
        groups.min_member[g] = lens[g] + int(groups.matched[g])
    return Case(bsa, soa, orc, (nodes, fit, groups, pods))


def of_case(c, bound, bits=None, wait=True):
    """B over a Case (one pass ran): the bound table loaded, the empty wait table loaded"""
    S = c.nodes.lanes - 4
    c.ctx.load_bound(bound)
    if bits is not None:
        c.ctx.bound_pdb_set(bits)
    if wait:
        c.ctx.wait_load()
    tab = wr.load(c.nodes.n, c.groups.g, S) if wait else None
    return B(c.ctx, c.soa, bar.Table(bound, S, c.nodes.n, bits=bits), tab, c.nodes.n, c.groups.g, pods=c.pods, pod_node=c.s["pod_node"].astype(np.int32),
             wait_node=c.st.wait_node, window=True)


def three_valued(rng, n_nodes, b, S, node=None):
    return bbr.make_bound(rng.integers(0, n_nodes, b) if node is None else np.full(b, node), rng.integers(0, 3, b), rng.integers(0, 3, b), S, rng)


# ---- the header's cycle, against a twin that binds the old way ---------------------------------------------------------------------------
def old_way(ctx, soa, S, released, pl, pod_node, pods, prio, start, pdb):
    """bs_wait_read + bs_wait_release + pod_node + host marshalling + bs_bound_apply: what bs_bound_bind replaces"""
    tab = ctx.wait_read()
    rel = ctx.wait_release(released)
    at = {int(v): e for e, v in enumerate(tab["id"])}
    e = [at[int(i)] for i in rel["id"]]
    node = np.concatenate([tab["node"][e], pod_node[pl].astype(np.uint32)])
    group = np.concatenate([tab["group"][e], pods.group[pl]])
    req = np.concatenate([tab["req"][:, e], pods.req[:, pl]], axis=1)
    pres = np.concatenate([tab["req_present"][e], pods.req_present[pl]])
    first = ctx.bound_apply(None, soa.Bound(node, prio, start, group, np.ascontiguousarray(req), pres), pdb)
    return rel["id"], first


@pytest.mark.parametrize("S", [0, 1, 12])
def test_the_cycle_equals_the_old_way_on_a_twin(S, bsa, soa, orc):
    """gangs of 1, 2, 63, 64 and 65 pods on 8 nodes, two passes: pass 1 leaves all 195 waiting (parked), pass 2 completes gangs 0, 2 and 4,
    whose earlier members are wait rows; release -> bind -> park -> a preemption whose victims include just-bound entries"""
    lens, P1 = [1, 2, 63, 64, 65], soa.STAGE_PREFILTER
    nodes, fit, groups, pods1 = waiting_scene(soa, lens, n_nodes=8, S=S, pods_cap=50, interleave=True, seed=200 + S)
    groups.min_member[[1, 3]] += 1                              # one more member is not enough for gangs 1 and 3
    rng = np.random.default_rng(300 + S)
    L = 4 + S
    group2 = np.array([0, 1, 2, 3, 4], np.int32)
    req2 = np.zeros((L, 5), np.int64)
    req2[0], req2[1] = rng.integers(1, 20, 5), rng.integers(1, 1 << 20, 5)
    pres2 = (rng.integers(0, 1 << S, 5) if S else np.zeros(5, np.int64)).astype(np.uint32)
    req2[4:] = rng.integers(1, 4, (S, 5)) * ((pres2[None, :] >> np.arange(S, dtype=np.uint32)[:, None]) & 1)
    pods2 = soa.Pods(group2, req2, pres2, np.zeros(5, np.uint32), np.zeros(5, np.uint64), np.zeros(5, np.uint8))
    bound = three_valued(rng, 8, 40, S)
    bound.priority[:] += 1                                      # 1..3: only a just-bound entry has priority 0
    bits = rng.integers(0, 2, 40)
    with Case(bsa, soa, orc, (nodes, fit, groups, pods1)) as a, Case(bsa, soa, orc, (nodes, fit, groups, pods1)) as b:
        assert int((a.st.wait_node >= 0).sum()) == 195
        for c in (a, b):
            c.ctx.load_bound(bound)
            c.ctx.bound_pdb_set(bits)
        wa, wb = W.of_case(a), W.of_case(b)
        pk = wa.park("A: park 1")
        wb.park("B: park 1")
        queue2 = wr.second_queue(soa, pods1, pk["pod"], pods2)
        s2 = orc.seq_replay(a.s["nodes"], fit, a.s["groups"], queue2, P1, leader=a.s["leader"])
        for w in (wa, wb):
            w.ctx.apply_pods(remove=pk["pod"], insert=pods2)
            r2 = w.ctx.seq_run(P1)
            assert np.array_equal(r2["pod_node"], s2["pod_node"]) and np.array_equal(r2["released_group"], s2["released_group"])
            w.st = ser.State.after_pass(a.s["nodes"], fit, a.s["groups"], queue2, s2)
            w.mg, w.pods = s2["groups"].copy(), queue2
            w.check("after pass 2")
        released = s2["released_group"].tolist()
        assert sorted(released) == [0, 2, 4]
        pod_node, waiting = s2["pod_node"].astype(np.int32), wa.st.wait_node.copy()          # (park 2 empties the model's)
        pl = np.nonzero(pod_node >= 0)[0]
        assert pl.size == 3 and int((waiting >= 0).sum()) == 2 and not np.any(waiting[pl] >= 0), "three placed pods completed their gangs, two still wait"
        wl = wa.tab.id[np.isin(wa.tab.group, released)]
        assert wl.size == 1 + 63 + 65
        n = wl.size + pl.size
        prio, start, pdb = rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int64), rng.integers(0, 2, n)
        # A: the new call; its wait rows in release order (ascending id)
        ba = B(a.ctx, soa, bar.Table(bound, S, 8, bits=bits), wa.tab, 8, 5, pods=queue2, pod_node=pod_node, wait_node=waiting, window=True)
        got = ba.bind("A: bind", wl, pl, prio, start, pdb)
        assert got["first_id"] == 40
        # B: the old way
        ids_b, first_b = old_way(b.ctx, soa, S, released, pl, pod_node, queue2, prio, start, pdb)
        assert np.array_equal(ids_b, wl) and first_b == 40
        wr.release(wb.tab, released, 8, 5)
        (ia, na), (ib, nb) = a.ctx.read_bound(), b.ctx.read_bound()
        assert ia.tobytes() == ib.tobytes() and na.tobytes() == nb.tobytes(), "ids and nodes of the two bound tables"
        da, db = a.ctx.bound_dump(), b.ctx.bound_dump()
        for f in bar.COLUMNS:
            assert da[f].tobytes() == db[f].tobytes(), f"column {f} of the two bound tables"
        assert (a.ctx.bound_ids(), a.ctx.bound_count()) == (b.ctx.bound_ids(), b.ctx.bound_count()) == (40 + n, 40 + n)
        for w in (wa, wb):
            w.park("park 2")
        assert wa.tab.w == 2 + 64 + 2 and np.array_equal(a.ctx.wait_read()["id"], b.ctx.wait_read()["id"])
        # every node's pods lane is filled up: a preemptor of priority 1 needs a victim of priority 0, which only a just-bound entry has
        for w in (wa, wb):
            w.ctx.assume_nodes([(k, [*w.st.requested[:3, k], 50, *w.st.requested[4:, k]], int(w.st.requested_present[k])) for k in range(8)])
        pre = np.nonzero(waiting >= 0)[0]
        ra = a.ctx.preempt(pre, np.full(pre.size, 1, np.int32), np.zeros(5, np.uint8), victim_cap=64)
        rb = b.ctx.preempt(pre, np.full(pre.size, 1, np.int32), np.zeros(5, np.uint8), victim_cap=64)
        for f in ("node", "n_victims", "victims"):
            assert np.array_equal(ra[f], rb[f]), f"bs_preempt_run: {f}"
        vict = np.concatenate([ra["victims"][i, : int(ra["n_victims"][i])] for i in range(pre.size) if ra["node"][i] >= 0] or [np.zeros(0, np.uint32)])
        assert vict.size and np.any(vict >= 40), f"victims {vict} include just-bound entries (node {ra['node']}, candidates {ra['n_candidates']})"


# ---- the rank loop's 64-slot windows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("survivors", [0, 70])
@pytest.mark.parametrize("cnt", [1, 63, 64, 65, 130])
def test_one_node_receives_a_segment_around_the_windows(cnt, survivors, bsa, soa):
    """priorities and starts from 3 values each: ties between inserts and with survivors in every combination"""
    rng = np.random.default_rng(cnt * 100 + survivors)
    bound = three_valued(rng, 3, survivors, 1, node=1)
    b = rows_ctx(bsa, soa, 3, 1, np.full(cnt + 3, 1), rng.integers(0, 2, cnt + 3), bound, rng=rng, bits=rng.integers(0, 2, survivors) if survivors else None)
    with b.ctx:
        b.check("loaded")
        wl = rng.permutation(cnt + 3)[:cnt]
        b.bind("bind", wl, (), rng.integers(0, 3, cnt).astype(np.int32), rng.integers(0, 3, cnt).astype(np.int64), rng.integers(0, 2, cnt))
        assert b.tab.w == 3 and b.bt.count == survivors + cnt


# ---- BS_BOUND_MAX_PER_NODE ---------------------------------------------------------------------------------------------------------------
def test_capacity_exactly_the_limit_then_one_more(bsa, soa):
    rng = np.random.default_rng(9)
    bound = bbr.make_bound(np.zeros(2047, np.int64), rng.integers(0, 3, 2047), rng.integers(0, 3, 2047), 0)
    b = rows_ctx(bsa, soa, 2, 0, np.zeros(4, np.int64), np.zeros(4, np.int64), bound, rng=rng)
    with b.ctx:
        b.refused(bsa, "2047 + 2", bbr.CAPACITY, [0, 1])
        b.bind("2047 + 1", [2], (), [1], [1])
        assert b.bt.count == 2048
        b.refused(bsa, "2048 + 1", bbr.CAPACITY, [0])
        b.bind("the empty call", (), ())


def test_capacity_of_a_segment_alone(bsa, soa):
    """an empty node receives 2049 rows: the rank kernel's own check; 2048 are fine"""
    rng = np.random.default_rng(10)
    b = rows_ctx(bsa, soa, 2, 0, np.ones(2049, np.int64), np.zeros(2049, np.int64), bbr.make_bound([], [], [], 0), rng=rng)
    with b.ctx:
        b.refused(bsa, "0 + 2049", bbr.CAPACITY, np.arange(2049))
        b.bind("0 + 2048", rng.permutation(2049)[:2048], (), rng.integers(0, 3, 2048).astype(np.int32), rng.integers(0, 3, 2048).astype(np.int64))
        assert b.tab.w == 1


# ---- the scans' blocks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1023, 1024, 1025])
def test_wait_tables_around_the_scan_block(w, bsa, soa):
    rng = np.random.default_rng(w)
    b = rows_ctx(bsa, soa, 5, 1, rng.integers(0, 5, w), rng.integers(0, 2, w), three_valued(rng, 5, 30, 1), rng=rng)
    with b.ctx:
        wl = np.unique(np.concatenate([[0, w - 1], np.arange(0, w, 7)]))
        wl = rng.permutation(wl)
        b.bind("first, last and every 7th", wl, (), rng.integers(0, 3, wl.size).astype(np.int32), rng.integers(0, 3, wl.size).astype(np.int64))
        b.bind("the last row again, now at the tail", [int(b.tab.id[-1])], (), [2], [0])


@pytest.mark.parametrize("n_nodes", [1, 1024, 1025])
def test_node_counts_around_the_scan_block(n_nodes, bsa, soa):
    rng = np.random.default_rng(n_nodes)
    w = 90
    node = rng.integers(0, n_nodes, w)
    node[:3] = n_nodes - 1                                      # the last node of the last block has a segment
    b = rows_ctx(bsa, soa, n_nodes, 0, node, rng.integers(0, 2, w), three_valued(rng, n_nodes, 50, 0), rng=rng)
    with b.ctx:
        b.bind("bind", rng.permutation(w)[:80], (), rng.integers(0, 3, 80).astype(np.int32), rng.integers(0, 3, 80).astype(np.int64))


def test_257_listed_pods_and_only_pods(bsa, soa, orc):
    """a released gang of 257 pods on 3 nodes, listed in a shuffled order; no wait row, and no wait table at all"""
    rng = np.random.default_rng(257)
    with released_case(bsa, soa, orc, [257, 2], [0], n_nodes=3, S=1, pods_cap=100, seed=11) as c:
        b = of_case(c, three_valued(rng, 3, 20, 1), wait=False)
        pl = np.nonzero((b.pod_node >= 0) & (b.wait_node < 0))[0]
        assert pl.size == 257 and int((b.wait_node >= 0).sum()) == 2
        pl = rng.permutation(pl)
        b.bind("257 pods", (), pl, rng.integers(0, 3, 257).astype(np.int32), rng.integers(0, 3, 257).astype(np.int64), rng.integers(0, 2, 257))


# ---- the edges ---------------------------------------------------------------------------------------------------------------------------
def test_empty_bound_table_down_to_an_empty_wait_table_and_a_growing_scratch(bsa, soa):
    rng = np.random.default_rng(12)
    w = 700
    b = rows_ctx(bsa, soa, 4, 12, rng.integers(0, 4, w), rng.integers(0, 2, w), bbr.make_bound([], [], [], 12), rng=rng)
    with b.ctx:
        b.bind("into the empty table", [5], (), [1], [1])
        rest = rng.permutation(np.setdiff1d(np.arange(w), [5]))
        b.bind("the second call outgrows the first one's scratch", rest[:600], (), rng.integers(0, 3, 600).astype(np.int32), rng.integers(0, 3, 600).astype(np.int64))
        b.bind("down to the empty wait table", rest[600:], (), rng.integers(0, 3, 99).astype(np.int32), rng.integers(0, 3, 99).astype(np.int64))
        assert b.tab.w == 0 and b.ctx.wait_count() == 0 and b.bt.count == 700
        b.refused(bsa, "an id of the empty table", bbr.INVALID, [3])


def test_int64_extremes_and_a_present_scalar_lane_of_zero(bsa, soa):
    """columns move untouched: no arithmetic is done on them"""
    S, w = 2, 6
    req = np.array([[I64MIN, I64MAX, -1, 0, 1, I64MIN + 1], [I64MAX, I64MIN, I64MAX, I64MIN, 0, -1], [0, -1, I64MIN, I64MAX, 5, 5], [1] * 6,
                    [0, I64MAX, 0, I64MIN, 7, 0], [I64MIN, 0, 0, 0, 0, I64MAX]], np.int64)
    pres = np.array([1, 3, 1, 3, 0, 2], np.uint32)               # rows 0 and 2: lane 4 present with value 0
    rng = np.random.default_rng(13)
    bound = three_valued(rng, 2, 5, S)
    bound.req[0, 0], bound.req[1, 1] = I64MIN, I64MAX
    b = rows_ctx(bsa, soa, 2, S, [0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 0, 1], bound, req=req, pres=pres)
    with b.ctx:
        b.bind("extremes", [4, 0, 3, 1, 2], (), [0, 1, 2, 1, 0], [I64MAX, I64MIN, 0, I64MIN, I64MAX])
        t = b.bt.table()
        assert I64MIN in t["req"] and I64MAX in t["req"] and np.any((t["req_present"] & 1 == 1) & (t["req"][4] == 0))


# ---- every refusal of the errors paragraph -----------------------------------------------------------------------------------------------
REFUSALS = ["before_bound_load", "bound_node_count", "no_wait_table", "stale_wait_counts", "no_window", "sharded", "null_wait_ids", "null_pod_index", "null_priority",
            "null_start", "wait_id_out_of_range", "wait_id_dead", "wait_id_twice", "pod_index_out_of_range", "pod_index_twice", "pod_without_node", "pod_still_waits"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_everything_unchanged(what, bsa, soa, orc):
    """gangs 0 and 2 are released (placed, not waiting), gang 1 waits, and the last pods find no node"""
    capi = bsa.capi
    rng = np.random.default_rng(21)
    with released_case(bsa, soa, orc, [3, 4, 5], [0], n_nodes=2, S=1, pods_cap=5, seed=22) as c:
        b = of_case(c, three_valued(rng, 2, 9, 1), bits=rng.integers(0, 2, 9), wait=what != "no_wait_table")
        ctx, lib = c.ctx, c.ctx._lib
        placed = np.nonzero((b.pod_node >= 0) & (b.wait_node < 0))[0]
        nowhere = np.nonzero((b.pod_node < 0) & (b.wait_node < 0))[0]
        assert placed.size == 3 and np.any(b.wait_node >= 0) and nowhere.size, "a pod that still waits and a pod without a node exist"
        if what != "no_wait_table":
            w = W(ctx, soa, c.orc, c.st, c.mg, b.tab, c.pods, window=True)
            w.park("park")
            b.wait_node = c.st.wait_node
            b.rebase()
            assert b.tab.w >= 4
            w.forget("one row dies", [1])
            b.rebase()
        wl, ok = [0, 2], placed[:2]
        one = (np.zeros(1, np.int32), np.zeros(1, np.int64))
        i32p, i64p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
        raw = lambda w_, p_, pr, st: lib.bs_bound_bind(ctx._h, 1 if w_ is not False else 0, w_ if w_ is not False else None, 1 if p_ is not False else 0,       # noqa: E731
                                                       p_ if p_ is not False else None, pr, st, None, None, None)
        z32, z64, zu = one[0].ctypes.data_as(i32p), one[1].ctypes.data_as(i64p), np.zeros(1, np.uint32).ctypes.data_as(u32p)
        if what == "before_bound_load":
            with load_ctx(bsa, c.nodes, c.fit, c.groups, c.pods) as fresh:
                fresh.wait_load()
                assert status_of(bsa, lambda: fresh.bound_bind((), (), (), ())) == bbr.STATE
            return
        if what == "bound_node_count":
            ctx.apply_node_deltas([_node_delta(bsa, c, capi.DELTA_APPEND, 0)])
            assert status_of(bsa, lambda: ctx.bound_bind(wl, (), *[x.repeat(2) for x in one])) == bbr.STATE
            assert status_of(bsa, lambda: ctx.bound_bind((), (), (), ())) == bbr.STATE
            _check_table(ctx, b.bt, "after the refusal")
            return
        if what == "stale_wait_counts":
            ctx.apply_node_deltas([_node_delta(bsa, c, capi.DELTA_APPEND, 0)])
            ctx.bound_nodes_apply([capi.DELTA_APPEND], [0])
            b.bt.n = 3
            assert status_of(bsa, lambda: ctx.bound_bind(wl, (), *[x.repeat(2) for x in one])) == bbr.STATE
            assert status_of(bsa, lambda: ctx.bound_bind((), ok, *[x.repeat(2) for x in one])) == bbr.STATE, "the APPEND ended the pass's window too"
            _check_table(ctx, b.bt, "after the refusal")
            return
        if what == "no_wait_table":
            b.refused(bsa, what, bbr.STATE, [0])
            b.bind("pods need no wait table", (), ok)
            return
        if what == "no_window":
            ctx.apply_pods(flag_index=[0], flag_value=[0])
            b.window = False
            b.rebase()
            b.refused(bsa, what, bbr.STATE, (), ok)
            b.bind("wait rows need no window", wl, ())
            return
        if what == "sharded":
            ctx.set_shard(0, 2)
            assert status_of(bsa, lambda: ctx.bound_bind(wl, ok, *[x.repeat(4) for x in one])) == bbr.STATE
            ctx.set_shard(0, 1)
            b.check("after the refusal")
        elif what == "null_wait_ids":
            assert raw(None, False, z32, z64) == bbr.INVALID
        elif what == "null_pod_index":
            assert raw(False, None, z32, z64) == bbr.INVALID
        elif what == "null_priority":
            assert raw(zu, False, None, z64) == bbr.INVALID
        elif what == "null_start":
            assert raw(zu, False, z32, None) == bbr.INVALID
        elif what == "wait_id_out_of_range":
            b.refused(bsa, what, bbr.INVALID, [0, b.tab.ids], ok)
        elif what == "wait_id_dead":
            b.refused(bsa, what, bbr.INVALID, [0, 1], ok)
        elif what == "wait_id_twice":
            b.refused(bsa, what, bbr.INVALID, [2, 0, 2], ok)
        elif what == "pod_index_out_of_range":
            b.refused(bsa, what, bbr.INVALID, wl, [int(ok[0]), c.pods.p])
        elif what == "pod_index_twice":
            b.refused(bsa, what, bbr.INVALID, wl, [int(ok[0]), int(ok[1]), int(ok[0])])
        elif what == "pod_without_node":
            b.refused(bsa, what, bbr.INVALID, wl, [int(ok[0]), int(nowhere[0])])
        elif what == "pod_still_waits":
            # the chains were emptied by the park: a fresh pass on a twin state shows the waiting pod
            with released_case(bsa, soa, orc, [3, 4, 5], [0], n_nodes=2, S=1, pods_cap=5, seed=22) as c2:
                b2 = of_case(c2, three_valued(rng, 2, 9, 1))
                assert np.any(b2.wait_node >= 0)
                b2.refused(bsa, what, bbr.INVALID, (), [int(placed[0]), int(np.nonzero(b2.wait_node >= 0)[0][0])])
                b2.bind("a correct call after the refusal", (), placed)
            return
        b.check(f"{what}: nothing changed")
        b.bind("a correct call after the refusal: the marks and the claim bitmap were left clean", wl, ok, [1, 0, 1, 2], [0, 1, 0, 2], [1, 0, 0, 1])


# ---- PDB ---------------------------------------------------------------------------------------------------------------------------------
def test_pdb_bits_given_null_and_the_resident_budgets_afterwards(bsa, soa):
    rng = np.random.default_rng(31)
    w, b0 = 12, 10
    bound = three_valued(rng, 3, b0, 0)
    b = rows_ctx(bsa, soa, 3, 0, rng.integers(0, 3, w), rng.integers(0, 2, w), bound, rng=rng, bits=np.zeros(b0, np.uint8))
    with b.ctx as ctx:
        # two budgets; every loaded entry is a member of budget 0, which is exhausted
        ctx.pdb_load([0, 5], np.arange(b0 + 1), np.zeros(b0, np.uint32))
        b.bt.pdb[:] = 1
        b.check("after bs_pdb_load")
        b.bind("bits given", [3, 1, 4], (), [1, 1, 2], [0, 0, 0], [1, 0, 1])
        b.bind("NULL: every bit clear", [5, 9], (), [0, 1], [2, 2], None)
        assert b.bt.pdb[b.bt.id >= b0].tolist() == [1, 0, 1, 0, 0]
        # a recompute: the new ids are not covered, they have no PDB
        ctx.pdb_allowed_apply([1], [4])
        b.bt.pdb[:] = (b.bt.id < b0).astype(np.uint8)
        b.check("bs_pdb_allowed_apply clears the uncovered ids")
        # the new ids become members of budget 1, which then runs out
        ctx.pdb_members_append(b0, np.arange(6), np.ones(5, np.uint32))
        ctx.pdb_allowed_apply([0, 1], [3, 0])
        b.bt.pdb[:] = (b.bt.id >= b0).astype(np.uint8)
        b.check("bs_pdb_members_append covers the new ids")


# ---- random sequences --------------------------------------------------------------------------------------------------------------------
def _groups_of(w):
    w.mg.matched[:] = w.st.matched
    w.mg.flags[:] = w.st.flags
    return w.mg


def _nodes_of(c, w):
    return c.soa.Nodes(c.nodes.allocatable, w.st.requested, c.nodes.allocatable_present, w.st.requested_present, c.nodes.flags)


FORCED_BINDS = (1, 7, 12)


@pytest.mark.parametrize("seed", range(20))
def test_random_sequences_against_the_two_models(seed, bsa, soa, orc):
    """park / release / bind / forget / bs_bound_apply / a pass on one context, 15 steps.  Steps 1, 7 and 12 bind one wait row and one
    placed pod, and the steps before them keep that many of each in reserve; step 13 is a second pass, step 14 binds from its results."""
    rng = np.random.default_rng(1000 + seed)
    S, N, P1 = int(seed % 3), 4, soa.STAGE_PREFILTER
    lens = [int(x) for x in rng.integers(2, 6, 4)]
    nodes, fit, groups, pods = waiting_scene(soa, lens, n_nodes=N, S=S, pods_cap=40, interleave=bool(seed % 2), seed=seed)
    for g in range(4):
        if g % 2 == seed % 2:
            groups.min_member[g] = lens[g]                      # these gangs are released by the first pass; the other two wait
    with Case(bsa, soa, orc, (nodes, fit, groups, pods)) as c:
        b = of_case(c, three_valued(rng, N, 12, S), bits=rng.integers(0, 2, 12))
        w = W(c.ctx, soa, c.orc, c.st, c.mg, b.tab, c.pods, window=True)
        s, bound_pods, both = c.s, set(), 0
        for step in range(15):
            reserve = sum(1 for f in FORCED_BINDS if f >= step)
            free = [int(p) for p in np.nonzero((b.pod_node >= 0) & (w.st.wait_node < 0))[0] if int(p) not in bound_pods]
            op = ("park" if step == 0 else "bind" if step in FORCED_BINDS or step == 14 else "pass" if step == 13 else
                  ["park", "bind", "forget", "apply", "release"][int(rng.integers(0, 5))])
            where = f"seed {seed} step {step} {op}"
            if op == "park":
                w.park(where)
                b.wait_node = w.st.wait_node
                b.rebase()
            elif op == "bind":
                if step in FORCED_BINDS:
                    assert b.tab.w and free, f"{where}: a wait row and a placed pod are left"
                    nw, npod = 1, 1
                else:
                    nw, npod = int(rng.integers(0, max(b.tab.w - reserve, 0) + 1)), int(rng.integers(0, max(len(free) - reserve, 0) + 1))
                wl, pl = rng.permutation(b.tab.id)[:nw], rng.permutation(free)[:npod] if npod else []
                n = len(wl) + len(pl)
                b.bind(where, wl, pl, rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int64), rng.integers(0, 2, n) if n and step % 2 else None)
                bound_pods.update(int(p) for p in pl)
                both += bool(len(wl) and len(pl))
            elif op == "forget" and b.tab.w > reserve:
                w.forget(where, [int(b.tab.id[int(rng.integers(0, b.tab.w))])])
                b.rebase()
            elif op == "release" and b.tab.w > reserve + 1:
                w.release(where, [int(b.tab.group[0])] if int((b.tab.group != b.tab.group[0]).sum()) >= reserve else [])
                b.check(where)
            elif op == "apply" and b.bt.count:
                rem = rng.permutation(b.bt.id)[: int(rng.integers(0, 3))]
                ins = three_valued(rng, N, int(rng.integers(0, 4)), S)
                b.bt.apply(rem, ins, None)
                c.ctx.bound_apply(rem, ins, None)
                b.check(where)
            elif op == "pass":
                # the same queue again on the state the model holds; the pods placed before keep their nodes' requests
                before = _nodes_of(c, w)
                s = orc.seq_replay(before, c.fit, _groups_of(w), c.pods, P1, leader=s["leader"])
                r = c.ctx.seq_run(P1)
                assert np.array_equal(r["pod_node"], s["pod_node"]), where
                w.st = ser.State.after_pass(before, c.fit, _groups_of(w), c.pods, s)
                w.mg = s["groups"].copy()
                b.pod_node, b.wait_node, bound_pods = s["pod_node"].astype(np.int32), w.st.wait_node, set()
                w.check(where)
                b.rebase()
                b.check(where)
        assert both >= 3, f"seed {seed}: {both} binds with both kinds of row"
