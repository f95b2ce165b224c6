"""GPU tests of the resident Permit-wait table, bs_wait_* (csrc/bs_wait.hpp), against the array model of tests/wait_ref.py, bit for bit.
After every call: bs_nodes_read, bs_groups_read, bs_find_max_pg (against the oracle on the model's groups), bs_wait_read / _count / _ids and,
while the pass's window is open, bs_seq_waiting_read."""
import numpy as np
import pytest

import seq_expire_ref as ser
import wait_ref as wr
from test_gpu_parity import load_ctx
from test_gpu_seq import assert_groups_equal
from test_gpu_seq_expire import Case, status_of, waiting_scene, _node_delta

pytestmark = pytest.mark.gpu
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


class W:
    """a context with a wait table, and the model of both: st (node requests, matched, flags, the pass's waiting pods), mg (the other group
    columns), tab"""

    def __init__(self, ctx, soa, orc, st, mg, tab, pods=None, window=False):
        self.ctx, self.soa, self.orc, self.st, self.mg, self.tab, self.pods, self.window = ctx, soa, orc, st, mg, tab, pods, window
        self.N, self.G = st.requested.shape[1], st.matched.size

    @staticmethod
    def of_case(c, load=True):
        if load:
            c.ctx.wait_load()
        return W(c.ctx, c.soa, c.orc, c.st, c.mg, wr.load(c.nodes.n, c.groups.g, c.nodes.lanes - 4) if load else None, c.pods, window=True)

    def check(self, where):
        req, pres = self.ctx.read_node_requests()
        assert np.array_equal(pres, self.st.requested_present), f"{where}: node request keys"
        bad = np.nonzero(req != self.st.requested)
        assert bad[0].size == 0, f"{where}: node requests differ first at lane {bad[0][0]} node {bad[1][0]}: {req[bad][0]} vs {self.st.requested[bad][0]}"
        self.mg.matched[:] = self.st.matched
        self.mg.flags[:] = self.st.flags
        assert_groups_equal(self.ctx.read_groups(), self.mg, self.soa, where)
        leader, _, panic = self.orc.find_max_pg(self.mg)
        assert self.ctx.find_max_pg() == (leader, panic), f"{where}: findMaxPG"
        if self.tab is not None:
            assert (self.ctx.wait_count(), self.ctx.wait_ids()) == (self.tab.w, self.tab.ids), f"{where}: count, ids"
            got = self.ctx.wait_read()
            for k, v in self.tab.columns().items():
                assert np.array_equal(got[k], v), f"{where}: table column {k}"
        if self.window:
            assert np.array_equal(self.ctx.seq_waiting_read(), self.st.wait_node), f"{where}: bs_seq_waiting_read"

    def _same(self, where, got, exp, cap, rows):
        assert got["n"] == exp["n"], f"{where}: n {got['n']} vs {exp['n']}"
        k = exp["n"] if cap is None else min(exp["n"], cap)
        for f in exp:
            if f != "n" and f != "first_id":
                assert np.array_equal(got[f], exp[f][:k] if f in rows else exp[f]), f"{where}: {f}"
        self.check(where)
        return exp

    def park(self, where, cap=None):
        exp = wr.park(self.st, self.tab, self.pods)
        got = self.ctx.wait_park(cap=cap)
        assert got["first_id"] == exp["first_id"], where
        return self._same(where, got, exp, cap, ("pod", "node"))

    def release(self, where, groups, cap=None):
        return self._same(where, self.ctx.wait_release(groups, cap=cap), wr.release(self.tab, groups, self.N, self.G), cap, ("id", "node"))

    def expire(self, where, groups, deny=False, cap=None):
        return self._same(where, self.ctx.wait_expire(groups, deny=deny, cap=cap), wr.expire(self.st, self.tab, groups, deny=deny), cap, ("id", "node"))

    def forget(self, where, ids):
        exp = wr.forget(self.st, self.tab, ids)
        assert np.array_equal(self.ctx.wait_forget(ids), exp), f"{where}: node_out"
        self.check(where)


# ---- twin contexts: park + wait_expire == bs_seq_expire --------------------------------------------------------------------------------
@pytest.mark.parametrize("S,interleave,deny", [(0, False, True), (0, True, False), (1, True, True), (1, False, False), (12, True, True), (12, False, False)])
def test_park_then_expire_equals_seq_expire_on_a_twin(S, interleave, deny, bsa, soa, orc):
    """gangs of 1, 2, 63, 64 and 65 pods on 8 nodes that hold 50 pods each: all 195 wait, on four nodes, and gangs share nodes; group 1 is closed, three groups enter with matched > 0"""
    scene = waiting_scene(soa, [1, 2, 63, 64, 65], n_nodes=8, S=S, pods_cap=50, interleave=interleave, matched0=[1, 0, 2, 0, 3], closed=(1,), seed=100 + S)
    with Case(bsa, soa, orc, scene) as a, Case(bsa, soa, orc, scene) as b:
        wait = a.st.wait_node.copy()
        assert int((wait >= 0).sum()) == 195 and len({(int(wait[i]), int(a.pods.group[i])) for i in range(195)}) > len(set(wait.tolist())), "gangs share nodes"
        w = W.of_case(b)
        w.check("empty table")
        pk = w.park("park")
        assert pk["n"] == 195 and np.all(b.ctx.seq_waiting_read() == -1)
        nothing = b.ctx.seq_expire(all=True)
        assert (nothing["n_groups"], nothing["n_pods"]) == (0, 0), "the chains are empty: a bs_seq_expire forgets nothing"
        w.check("bs_seq_expire(ALL) after the park")
        for glist in ([4, 1, 0], [2, 3]):
            ea = a.expire(f"A {glist}", groups=glist, deny=deny)
            eb = w.expire(f"B {glist}", glist, deny=deny)
            assert np.array_equal(eb["group_entries"], ea["group_pods"]) and np.array_equal(eb["group_unknown"], ea["group_earlier"])
            rows = sorted(zip(pk["pod"][eb["id"] - pk["first_id"]].tolist(), eb["node"].tolist()))
            assert rows == sorted(zip(ea["pod"].tolist(), ea["node"].tolist())), "B's rows map to A's (pod, node)"
            (qa, pa), (qb, pb) = a.ctx.read_node_requests(), b.ctx.read_node_requests()
            assert np.array_equal(qa, qb) and np.array_equal(pa, pb), "node requests and key bits"
            assert_groups_equal(a.ctx.read_groups(), b.ctx.read_groups(), soa, "group state")
        assert w.tab.w == 0 and np.array_equal(a.st.requested, b.st.requested)


# ---- two real cycles on one context -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4, 7, 10, 17])
def test_two_cycles_on_one_context(seed, bsa, soa, orc):
    nodes, fit, groups, pods1, pods2, _ = wr.two_cycle_scene(soa, seed)
    P = soa.STAGE_PREFILTER
    with Case(bsa, soa, orc, (nodes, fit, groups, pods1)) as c:
        ctx, s1 = c.ctx, c.s
        w = W.of_case(c)
        pk1 = w.park("cycle 1: park")
        wait1 = np.full(pods1.p, -1, np.int64)
        wait1[pk1["pod"]] = pk1["node"]
        ctx.apply_pods(remove=pk1["pod"], insert=pods2)
        queue2 = wr.second_queue(soa, pods1, pk1["pod"], pods2)
        got = ctx.read_pods()
        assert np.array_equal(got.group, queue2.group) and np.array_equal(got.req, queue2.req), "the queue of cycle 2"
        s2 = orc.seq_replay(s1["nodes"], fit, s1["groups"], queue2, P, leader=s1["leader"])
        r2 = ctx.seq_run(P)
        for name in ("pf_code", "pod_node", "released_group", "released_pods", "n_released"):
            assert np.array_equal(r2[name], s2[name]), f"pass 2: {name}"
        w.st = ser.State.after_pass(s1["nodes"], fit, s1["groups"], queue2, s2)
        w.mg, w.pods = s2["groups"].copy(), queue2
        w.check("after pass 2")
        released = s2["released_group"].tolist()
        rel = w.release("cycle 2: release", released)
        want = [(int(i), int(wait1[i])) for i in np.nonzero(wait1 >= 0)[0] if int(pods1.group[i]) in released]
        assert list(zip(pk1["pod"][rel["id"] - pk1["first_id"]].tolist(), rel["node"].tolist())) == want, "pass 1's (pod -> node) of the released gangs"
        pk2 = w.park("cycle 2: park")
        assert pk2["first_id"] == pk1["n"]
        short = sorted(set(w.tab.group.tolist()))
        if short:
            w.expire("cycle 2: a short gang times out", [short[seed % len(short)]], deny=True)
        if w.tab.w:
            w.forget("cycle 2: one more pod is deleted", [int(w.tab.id[w.tab.w // 2])])
        # a batch and a third pass answer as a twin that ran the same passes (same sop.maxFinishedPG) and then LOADED the model's state
        with load_ctx(bsa, nodes, fit, groups, pods1) as twin:
            twin.seq_run(P)
            twin.apply_pods(remove=pk1["pod"], insert=pods2)
            twin.seq_run(P)
            twin.load_nodes(soa.Nodes(nodes.allocatable, w.st.requested, nodes.allocatable_present, w.st.requested_present, nodes.flags), fit)
            w.mg.matched[:], w.mg.flags[:] = w.st.matched, w.st.flags
            twin.load_groups(w.mg)
            twin.load_pods(queue2)
            x, y = ctx.batch(soa.STAGE_ALL, bitmap=False), twin.batch(soa.STAGE_ALL, bitmap=False)
            for name in ("pf_code", "pf_first_k", "pf_leader", "fl_code", "fl_feasible", "group_admit", "group_ready"):
                assert np.array_equal(getattr(x, name), getattr(y, name)), f"batch after the cycle: {name}"
            ra, rb = ctx.seq_run(P), twin.seq_run(P)
            for name in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods", "n_released"):
                assert np.array_equal(ra[name], rb[name]), f"third pass: {name}"
            (qa, pa), (qb, pb) = ctx.read_node_requests(), twin.read_node_requests()
            assert np.array_equal(qa, qb) and np.array_equal(pa, pb), "node requests after the third pass"
            assert_groups_equal(ctx.read_groups(), twin.read_groups(), soa, "groups after the third pass")
            assert np.array_equal(ctx.seq_waiting_read(), twin.seq_waiting_read())


# ---- block boundaries: the two-level scan, the compaction, the dirty list ---------------------------------------------------------------
def loaded(bsa, soa, orc, rows, S=2, seed=0, extremes=False):
    """a context on 24 nodes and 5 groups with a table of `rows` entries set up by wait_load; group 4 has no entry, the last entry is group 3's"""
    rng = np.random.default_rng(seed + rows)
    nodes, fit, groups, pods = waiting_scene(soa, [1, 1, 1, 1, 1], n_nodes=24, S=S, matched0=[3, 0, 2, 1, 5], seed=seed)
    nodes.requested_present[:] = (1 << S) - 1
    L = 4 + S
    node = rng.integers(0, 24, rows).astype(np.uint32)
    group = rng.integers(0, 4, rows).astype(np.int32)
    group[-1] = 3
    req = rng.integers(0, 1000, (L, rows)).astype(np.int64)
    if extremes:
        req[0] = rng.choice([I64MIN, I64MAX, I64MIN + 1, -1, 1], rows)
        req[1] = rng.choice([I64MAX, I64MIN], rows)
        node[: rows // 2] = 5                                       # many extreme rows on one node: the sums wrap several times
        if S:
            req[4] = rng.choice([I64MIN, I64MAX, 7], rows)
    pres = (rng.integers(0, 1 << S, rows) if S else np.zeros(rows, np.int64)).astype(np.uint32)
    ctx = load_ctx(bsa, nodes, fit, groups, pods)
    st = ser.State(nodes.requested, nodes.requested_present, groups.matched, groups.flags, np.zeros(0, np.int32))
    w = W(ctx, soa, orc, st, groups.copy(), None, pods)
    cols = (node, group, req, pres)

    def reload():
        ctx.wait_load(*cols)
        w.tab = wr.load(24, 5, S, *cols)
    reload()
    return w, reload


@pytest.mark.parametrize("rows", [1, 1023, 1024, 1025, 2100])
def test_table_sizes_around_the_scan_block(rows, bsa, soa, orc):
    w, reload = loaded(bsa, soa, orc, rows, seed=rows)
    with w.ctx:
        w.check(f"{rows}: loaded")
        last = int(w.tab.group[-1])
        for op in ("release", "expire"):
            for name, glist in (("nothing", [4]), ("all", [3, 0, 4, 2, 1]), ("every second group", [0, 2, 4]), ("the last entry's group", [last])):
                where = f"{rows} rows, {op} {name}"
                before = w.tab.w
                e = w.release(where, glist) if op == "release" else w.expire(where, glist, deny=name == "all")
                assert e["n"] == {"nothing": 0, "all": before}.get(name, e["n"]) and (name == "nothing" or rows < 1023 or e["n"] >= 100)
                reload()
                w.check(f"{where}: reloaded")
        for name, ids in (("both ends", sorted({rows - 1, 0}, reverse=True)), ("across the block boundary", [i for i in (1024, 1022, 1023, 1025) if i < rows]), ("every row", list(range(rows)))):
            if not ids:
                continue
            w.forget(f"{rows} rows, forget {name}", ids)
            if name == "both ends" and rows > 2:
                w.forget(f"{rows} rows, forget the new ends", [1, rows - 2])
                assert status_of(bsa, lambda: w.ctx.wait_forget([0])) == -1, "a dead id"
                w.check("after the dead id")
            reload()


@pytest.mark.parametrize("S", [0, 1])
def test_int64_extremes_wrap(S, bsa, soa, orc):
    w, reload = loaded(bsa, soa, orc, 40, S=S, seed=5, extremes=True)
    with w.ctx:
        w.expire("extremes: two gangs", [1, 3], deny=True)
        w.forget("extremes: single rows", [int(x) for x in w.tab.id[::3]])
        w.expire("extremes: the rest", [0, 2])
        assert w.tab.w == 0


def test_scratch_that_grows_between_two_removal_calls_is_zero_again(bsa, soa, orc):
    """the mark arrays (by group, by id) and the per-node sums are zero between calls and are allocated for what the first removal call
    needs (256 marks, 24 nodes).  On the SAME context the id space, the group count and the node count then grow past that: the blocks are
    allocated again — possibly at their old address — and must be zeroed again, or rows of groups and ids nobody listed would leave"""
    w, _ = loaded(bsa, soa, orc, 40, seed=9)
    ctx = w.ctx
    with ctx:
        w.forget("small: forget", [3, 39])
        w.expire("small: expire", [1], deny=True)
        w.release("small: release", [0])
        rng = np.random.default_rng(77)
        G, N, rows, S = 600, 700, 3000, 2
        nodes, fit, groups, pods = waiting_scene(soa, [1] * G, n_nodes=N, S=S, matched0=[int(x) for x in rng.integers(0, 4, G)], seed=78)
        nodes.requested_present[:] = (1 << S) - 1
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        cols = (rng.integers(0, N, rows).astype(np.uint32), rng.integers(0, G, rows).astype(np.int32), rng.integers(0, 1000, (4 + S, rows)).astype(np.int64),
                rng.integers(0, 1 << S, rows).astype(np.uint32))
        ctx.wait_load(*cols)
        big = W(ctx, soa, orc, ser.State(nodes.requested, nodes.requested_present, groups.matched, groups.flags, np.zeros(0, np.int32)), groups.copy(),
                wr.load(N, G, S, *cols), pods)
        big.check("grown: loaded")
        big.forget("grown: ids beyond the first mark block", [2999, 300, 5, 257])
        assert big.tab.w == rows - 4
        e = big.expire("grown: groups beyond the first mark block", [599, 300, 1, 256], deny=True)
        assert e["n"] == int(np.isin(cols[1], [599, 300, 1, 256]).sum()) - int(np.isin(cols[1][[2999, 300, 5, 257]], [599, 300, 1, 256]).sum())
        big.release("grown: release", [2, 400, 598])
        big.forget("grown: forget again", [int(x) for x in big.tab.id[::97]])
        big.expire("grown: every group", rng.permutation(G))
        assert big.tab.w == 0


# ---- capacities -------------------------------------------------------------------------------------------------------------------------
def test_a_park_that_would_pass_the_id_space_is_refused_whole(bsa, soa, orc):
    """a table of exactly BS_WAIT_MAX rows (the only way to the edge of the id space: ids never shrink): the park of five waiting pods is
    BS_ERR_CAPACITY and the table's counts, the chains, the nodes and the groups are as before; with room again the same park succeeds"""
    M = bsa.capi.WAIT_MAX
    with Case(bsa, soa, orc, waiting_scene(soa, [3, 2], n_nodes=3, seed=41)) as c:
        ctx = c.ctx
        ctx.wait_load(np.zeros(M, np.uint32), np.zeros(M, np.int32), np.zeros((4, M), np.int64), np.zeros(M, np.uint32))
        assert (ctx.wait_count(), ctx.wait_ids()) == (M, M)
        assert status_of(bsa, ctx.wait_park) == -5
        assert (ctx.wait_count(), ctx.wait_ids()) == (M, M)
        c.check_state("after the refused park")                       # nodes, groups, findMaxPG and the chains (bs_seq_waiting_read)
        w = W.of_case(c)                                             # the empty table: there is room again
        assert w.park("park with room")["n"] == 5


def test_caps_below_the_true_count_truncate_the_rows_only(bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [4, 3, 5], n_nodes=3, interleave=True, seed=21)) as c:
        w = W.of_case(c)
        assert w.park("park, cap 2", cap=2)["n"] == 12
        assert w.release("release, cap 1", [1], cap=1)["n"] == 3
        assert w.expire("expire, cap 0", [0], cap=0)["n"] == 4
        assert w.expire("expire, cap 3", [2], cap=3, deny=True)["n"] == 5 and w.tab.w == 0


# ---- errors: nothing resident changes ---------------------------------------------------------------------------------------------------
def test_every_refused_call_leaves_the_state_alone(bsa, soa, orc):
    capi = bsa.capi
    with Case(bsa, soa, orc, waiting_scene(soa, [3, 2, 2], n_nodes=3, S=1, seed=43)) as c:
        ctx = c.ctx
        for fn in (ctx.wait_count, ctx.wait_ids, ctx.wait_read, ctx.wait_park, lambda: ctx.wait_release([0]), lambda: ctx.wait_expire([0]), lambda: ctx.wait_forget([0])):
            assert status_of(bsa, fn) == -4, "no table"
        w = W.of_case(c)
        w.park("park")
        assert w.park("park twice")["n"] == 0
        w.forget("one id dies", [2])
        n = capi.C.c_uint32(0)
        for where, want, fn in [("group >= g", -1, lambda: ctx.wait_release([0, 3])),
                                ("group listed twice (release)", -1, lambda: ctx.wait_release([1, 0, 1])),
                                ("group listed twice (expire)", -1, lambda: ctx.wait_expire([2, 2])),
                                ("more groups than there are", -1, lambda: ctx.wait_expire([0, 1, 2, 0])),
                                ("unknown flag bits", -1, lambda: ctx.wait_expire([0], flags=2)),
                                ("a dead id", -1, lambda: ctx.wait_forget([2])),
                                ("a dead id among live ones", -1, lambda: ctx.wait_forget([0, 2, 1])),
                                ("an id listed twice", -1, lambda: ctx.wait_forget([1, 3, 1])),
                                ("an id beyond the id space", -1, lambda: ctx.wait_forget([7])),
                                ("NULL list with a count", -1, lambda: ctx._chk(ctx._lib.bs_wait_release(ctx._h, 2, None, 0, None, None, None, capi.C.byref(n)), "bs_wait_release")),
                                ("NULL rows with a cap", -1, lambda: ctx._chk(ctx._lib.bs_wait_park(ctx._h, 4, None, None, capi.C.byref(n), capi.C.byref(n)), "bs_wait_park")),
                                ("a load beyond BS_WAIT_MAX", -5, lambda: ctx.wait_load([0], [0], w=capi.WAIT_MAX + 1)),
                                ("a load with a node >= n", -1, lambda: ctx.wait_load([0, 3], [0, 0])),
                                ("a load with a group >= g", -1, lambda: ctx.wait_load([0, 1], [0, 3])),
                                ("a load with a negative group", -1, lambda: ctx.wait_load([0, 1], [0, -1]))]:
            assert status_of(bsa, fn) == want, where
            w.check(f"after the refused call: {where}")
        for fn in (lambda: ctx.wait_release([]), lambda: ctx.wait_expire([]), lambda: ctx.wait_forget([])):
            fn()                                                       # an empty list is no error and no change
            w.check("after an empty list")
        ctx.set_shard(0, 2)
        for fn in (ctx.wait_read, ctx.wait_park, lambda: ctx.wait_release([0]), lambda: ctx.wait_expire([0]), lambda: ctx.wait_forget([0]), ctx.wait_load):
            assert status_of(bsa, fn) == -4, "a sharded context"
        ctx.set_shard(0, 1)
        w.check("after the sharded calls")
        # ---- the pass's window: a queue patch ends it; the table lives on
        ctx.apply_pods(flag_index=[0], flag_value=[0])
        w.window = False
        assert status_of(bsa, ctx.wait_park) == -4, "park outside the window"
        w.check("after the park outside the window")
        # ---- stale counts: an APPEND changes the node count
        ctx.apply_node_deltas([_node_delta(bsa, c, capi.DELTA_APPEND, 0)])
        assert (ctx.wait_count(), ctx.wait_ids()) == (w.tab.w, w.tab.ids), "count and ids answer on a stale table"
        for fn in (ctx.wait_read, lambda: ctx.wait_release([0]), lambda: ctx.wait_expire([0]), lambda: ctx.wait_forget([0])):
            assert status_of(bsa, fn) == -4, "a stale node count"
        ctx.apply_node_deltas([_node_delta(bsa, c, capi.DELTA_REMOVE, 3)])
        w.check("the count is back: the table is valid again, and nothing of it changed")
        w.expire("and the state still expires", [0, 1, 2], deny=True)
        assert w.tab.w == 0
