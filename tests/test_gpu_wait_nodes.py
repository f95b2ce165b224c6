"""GPU tests of bs_wait_nodes_apply (csrc/bs_wait.hpp: k_wn_map, the spread scan's by-node face, k_wn_move): after bs_nodes_apply +
bs_wait_nodes_apply the resident wait table, its counts, the groups and the returned rows equal the array model of
tests/wait_nodes_ref.py, bit for bit; a twin context that took the host round trip the call replaces ends in the same state; a real cycle
under churn against the sequential oracle; the refusals leave everything alone."""
import ctypes as C

import numpy as np
import pytest

import bound_nodes_ref as bn
import seq_expire_ref as ser
import wait_nodes_ref as wn
import wait_ref as wr
from test_gpu_parity import load_ctx
from test_gpu_seq import assert_groups_equal
from test_gpu_seq_expire import Case, status_of, waiting_scene
from test_gpu_wait import W

pytestmark = pytest.mark.gpu
U, A, R = wn.UPDATE, wn.APPEND, wn.REMOVE


class WN(W):
    """test_gpu_wait.W plus the node list: bs_nodes_apply and bs_wait_nodes_apply on the context, and the model of both"""

    def __init__(self, ctx, soa, orc, st, mg, tab, nl, pods=None, window=False):
        super().__init__(ctx, soa, orc, st, mg, tab, pods, window)
        self.nl = nl

    def cut(self, steps, split=None):
        """bs_nodes_apply of steps = [(kind, index)], in one call or — split — in two; the model's node requests follow the list.
        -> (kinds, indices) of all deltas in order"""
        nl = self.nl
        nl.req, nl.rpres = self.st.requested.copy(), self.st.requested_present.copy()
        deltas = [nl.append(int(i) % len(nl.pool[1])) if k == A else nl.remove(int(i)) if k == R else nl.update(int(i)) for k, i in steps]
        for part in ([deltas] if split is None else [deltas[:split], deltas[split:]]):
            if part:
                self.ctx.apply_node_deltas(part)
        assert self.ctx.n == nl.n
        self.st.requested, self.st.requested_present = nl.req.copy(), nl.rpres.copy()
        self.N = nl.n
        if any(k != U for k, _ in steps):
            self.window = False
        return [d.kind for d in deltas], [d.index for d in deltas]

    def follow(self, where, kinds, idx, cap=None):
        exp = wn.nodes_apply(self.tab, self.st.matched, kinds, idx, n_expected=self.nl.n, g=self.G)
        ids, old, grp, n = self.ctx.wait_nodes_apply(kinds, idx, cap=cap)
        k = exp["n"] if cap is None else min(exp["n"], cap)
        assert n == exp["n"], f"{where}: n {n}, the model drops {exp['n']}"
        assert np.array_equal(ids, exp["id"][:k]) and np.array_equal(old, exp["node"][:k]) and np.array_equal(grp, exp["group"][:k]), f"{where}: the rows"
        self.check(where)
        return exp

    def surgery(self, where, steps, cap=None, split=None):
        return self.follow(where, *self.cut(steps, split), cap=cap)

    def run_pass(self, where, queue, leader):
        """bs_seq_run over `queue` (the context's queue) against the oracle on the model's nodes and groups; the window opens.  -> the oracle's pass"""
        P = self.soa.STAGE_PREFILTER
        self.mg.matched[:], self.mg.flags[:] = self.st.matched, self.st.flags
        nodes, fit = self.nl.nodes(self.st.requested, self.st.requested_present), self.nl.fit()
        s = self.orc.seq_replay(nodes, fit, self.mg, queue, P, leader=leader)
        r = self.ctx.seq_run(P)
        for name in ("pf_code", "pod_node", "released_group", "released_pods", "n_released"):
            assert np.array_equal(r[name], s[name]), f"{where}: {name}: {r[name]} vs {s[name]}"
        self.st = ser.State.after_pass(nodes, fit, self.mg, queue, s)
        self.mg, self.pods, self.window = s["groups"].copy(), queue, True
        self.check(where)
        return s


def table_ctx(bsa, soa, orc, N, G, S, cols, matched0, seed=0):
    """a context on N nodes and G groups whose table was set up by wait_load(cols); -> (WN, reload)"""
    nodes, fit, groups, pods = waiting_scene(soa, [1] * G, n_nodes=N, S=S, matched0=[int(x) for x in matched0], seed=seed)
    nodes.requested_present[:] = (1 << S) - 1
    ctx = load_ctx(bsa, nodes, fit, groups, pods)
    ctx.wait_load(*cols)

    def state():
        return ser.State(nodes.requested, nodes.requested_present, groups.matched, groups.flags, np.zeros(0, np.int32))
    w = WN(ctx, soa, orc, state(), groups.copy(), wr.load(N, G, S, *cols), bn.NodeList(nodes, fit), pods)

    def reload():
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(groups)
        ctx.wait_load(*cols)
        w.st, w.mg, w.tab, w.nl, w.N = state(), groups.copy(), wr.load(N, G, S, *cols), bn.NodeList(nodes, fit), N
    return w, reload


def columns(rng, rows, N, G, S):
    """rows on random nodes in random groups; every seventh row belongs to the last group and sits on node 7"""
    node = rng.integers(0, N, rows).astype(np.uint32)
    group = rng.integers(0, G - 1, rows).astype(np.int32)
    sel = np.arange(rows) % 7 == 0
    node[sel], group[sel] = 7, G - 1
    pres = (rng.integers(0, 1 << S, rows) if S else np.zeros(rows, np.int64)).astype(np.uint32)
    return node, group, rng.integers(0, 1000, (4 + S, rows)).astype(np.int64), pres


def remove_steps(rng, old):
    """(REMOVE, current index) for the OLD nodes `old`, in a random order (valid while no REMOVE of another node comes in between)"""
    gone, steps = [], []
    for k in rng.permutation(sorted(old)):
        steps.append((R, int(k) - sum(x < k for x in gone)))
        gone.append(int(k))
    return steps


# ---- the model: table sizes around the scan block x lengths of the removed list ----------------------------------------------------------
@pytest.mark.parametrize("rows,S", [(1, 0), (1023, 1), (1024, 12), (1025, 1), (2100, 0)])
def test_table_and_groups_equal_the_model(rows, S, bsa, soa, orc):
    N, G = 130, 6
    rng = np.random.default_rng(rows)
    cols = columns(rng, rows, N, G, S)
    gang = int((cols[1] == G - 1).sum())
    if rows == 2100:
        at = np.nonzero(cols[1] == G - 1)[0]
        assert gang >= 300 and {0, 1, 2} <= set((at // 1024).tolist()), "one gang of 300 rows in three scan blocks, all on node 7"
        assert len(set(cols[1][cols[0] == 7].tolist())) >= 3, "rows of three groups on one removed node"
    w, reload = table_ctx(bsa, soa, orc, N, G, S, cols, rng.integers(0, 3, G), seed=rows)
    with w.ctx:
        w.check(f"{rows}: loaded")
        for length in (0, 1, 64, 65, "all"):
            where = f"{rows} rows, {length} nodes removed"
            if length == 0:
                steps = [(U, 3), (A, 1), (A, 2), (U, N + 1)]
            elif length == 1:
                steps = [(R, 7)]
            elif length == "all":
                steps = [(A, 9)] + remove_steps(rng, range(N))
            else:
                others = rng.permutation([k for k in range(1, N - 1) if k != 7])[: length - 3].tolist()
                steps = [(A, 5)] + remove_steps(rng, [0, 7, N - 1] + others) + [(U, 0)]           # node 0, the last node, node 7 and others
            e = w.surgery(where, steps)
            assert w.ctx.wait_ids() == rows
            if length == 0:
                assert e["n"] == 0 and w.N == N + 2
            else:
                assert e["n"] >= gang and not np.any(w.tab.group == G - 1), "the whole gang on node 7 left, from every block"
            if length == "all":
                assert e["n"] == rows and w.tab.w == 0 and w.N == 1
            if length in (0, 64) and w.tab.w:                                  # the table lives on: the removal core on the new list
                w.expire(f"{where}: expire afterwards", [0, G - 1], deny=True)
                if w.tab.w:
                    w.forget(f"{where}: forget afterwards", [int(w.tab.id[0])])
            reload()
            w.check(f"{where}: reloaded")


# ---- a twin that takes the host round trip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1, 12])
def test_a_twin_that_reads_remaps_and_loads_ends_in_the_same_state(S, bsa, soa, orc):
    N, G, rows = 40, 5, 300
    rng = np.random.default_rng(50 + S)
    node, group = rng.integers(0, N, rows).astype(np.uint32), rng.integers(0, G, rows).astype(np.int32)
    pres = (rng.integers(0, 1 << S, rows) if S else np.zeros(rows, np.int64)).astype(np.uint32)
    cols = (node, group, rng.integers(0, 1000, (4 + S, rows)).astype(np.int64), pres)
    matched0 = np.bincount(group, minlength=G)                                 # a caller that parks every cycle: matched counts the rows
    a, _ = table_ctx(bsa, soa, orc, N, G, S, cols, matched0, seed=3)
    b, _ = table_ctx(bsa, soa, orc, N, G, S, cols, matched0, seed=3)
    with a.ctx, b.ctx:
        before = a.tab.copy()
        read_b = b.ctx.wait_read()                                             # the old path reads BEFORE the surgery: afterwards the count is stale
        steps = [(R, 0), (A, 1), (R, 38), (U, 2), (R, 10), (R, 10), (A, 2), (R, 37)]      # (R, 37) names the second appended node and cancels it
        kinds, idx = a.cut(steps)
        b.ctx.apply_node_deltas(_deltas_again(b, steps))
        exp = a.follow(f"S={S}: the new path", kinds, idx)
        new, n_new = wn.by_identity(N, before.node, kinds, idx)
        assert n_new == a.N == b.ctx.n and exp["n"] == int((new < 0).sum()) > 0
        assert np.array_equal(a.ctx.wait_read()["id"], before.id[new >= 0]), "the ids on the new path are the survivors' old ids"
        load_cols, dropped_groups = wn.remap_on_the_host(read_b, N, kinds, idx)
        b.ctx.wait_load(*load_cols)
        gb = b.ctx.read_groups()
        fell = np.bincount(dropped_groups, minlength=G)
        b.ctx.apply_group_deltas([(g, (int(gb.matched[g]) - int(fell[g])) & 0xFFFFFFFF, int(gb.status_scheduled[g]), int(gb.flags[g])) for g in range(G) if fell[g]])
        ta, tb = a.ctx.wait_read(), b.ctx.wait_read()
        for f in ("node", "group", "req", "req_present"):
            assert np.array_equal(ta[f], tb[f]), f"S={S}: column {f}"
        assert np.array_equal(tb["id"], np.arange(tb["id"].size)) and a.ctx.wait_count() == b.ctx.wait_count()

        def same(what):
            (qa, pa), (qb, pb) = a.ctx.read_node_requests(), b.ctx.read_node_requests()
            assert np.array_equal(qa, qb) and np.array_equal(pa, pb), f"S={S}: node requests {what}"
            assert_groups_equal(a.ctx.read_groups(), b.ctx.read_groups(), soa, f"S={S}: group state {what}")
            assert a.ctx.find_max_pg() == b.ctx.find_max_pg()
        same("after the surgery")
        every = list(range(G))
        ea = a.expire(f"S={S}: expire of every group", every, deny=True)
        eb = b.ctx.wait_expire(every, deny=True)
        assert eb["n"] == ea["n"] and np.array_equal(eb["node"], ea["node"]) and np.array_equal(eb["group_entries"], ea["group_entries"])
        assert not np.any(ea["group_unknown"]) and not np.any(eb["group_unknown"]), "group_unknown == 0 on both paths"
        same("after the expire")


def _deltas_again(w, steps):
    """the same steps on a second context's own node list (its model state is not followed)"""
    nl = w.nl
    nl.req, nl.rpres = w.st.requested.copy(), w.st.requested_present.copy()
    return [nl.append(int(i) % len(nl.pool[1])) if k == A else nl.remove(int(i)) if k == R else nl.update(int(i)) for k, i in steps]


# ---- a real cycle under churn ----------------------------------------------------------------------------------------------------------------
def test_a_real_cycle_under_churn(bsa, soa, orc):
    """cycle 1: pass + park.  Surgery: a node that holds rows and three that hold none leave, four are appended.  bs_wait_nodes_apply.
    Cycle 2 on the new list leaves pods waiting on appended nodes; release, park, expire with deny: node requests, groups and table equal
    the model at every step (the per-node scratch and the dirty list on nodes beyond the old nodes)"""
    nodes, fit, groups, pods1, pods2, steps = wn.churn_scene(soa)
    with Case(bsa, soa, orc, (nodes, fit, groups, pods1)) as c:
        ctx = c.ctx
        ctx.wait_load()
        w = WN(ctx, soa, orc, c.st, c.mg, wr.load(nodes.n, groups.g, nodes.lanes - 4), bn.NodeList(nodes, fit), pods1, window=True)
        pk1 = w.park("cycle 1: park")
        assert pk1["n"] == 15
        out = w.surgery("the surgery", steps)
        assert out["n"] == 6 and set(out["node"].tolist()) == {0} and len(set(out["group"].tolist())) == 2 and w.N == 6
        ctx.apply_pods(remove=pk1["pod"], insert=pods2)
        queue2 = wr.second_queue(soa, pods1, pk1["pod"], pods2)
        s2 = w.run_pass("cycle 2: the pass", queue2, c.s["leader"])
        assert s2["n_released"] >= 1 and np.any(w.st.wait_node >= 2), "a gang is released, pods wait on appended nodes"
        rel = w.release("cycle 2: release", s2["released_group"].tolist())
        assert rel["n"] >= 1 and np.all(rel["node"] < 2), "the released rows name the old nodes' new indices"
        pk2 = w.park("cycle 2: park")
        assert pk2["first_id"] == 15 and np.any(w.tab.node >= 2)
        w.forget("cycle 2: a pod on an appended node is deleted", [int(w.tab.id[np.nonzero(w.tab.node >= 2)[0][0]])])
        ex = w.expire("cycle 2: the short gangs time out", sorted(set(w.tab.group.tolist())), deny=True)
        assert w.tab.w == 0 and ex["n"] >= 2 and not np.any(ex["group_unknown"])


def test_the_per_node_scratch_after_the_node_count_grew(bsa, soa, orc):
    """the removal core's per-node scratch ([L][N] sums, key bits, dirty words) is allocated by the first expire, for 24 nodes.  The list then
    grows to 700 nodes through bs_nodes_apply + bs_wait_nodes_apply: the next expire and forget find it large enough and zero"""
    N, G, S, rows = 24, 5, 2, 60
    rng = np.random.default_rng(8)
    cols = (rng.integers(0, N, rows).astype(np.uint32), rng.integers(0, G, rows).astype(np.int32), rng.integers(0, 1000, (4 + S, rows)).astype(np.int64),
            rng.integers(0, 1 << S, rows).astype(np.uint32))
    w, _ = table_ctx(bsa, soa, orc, N, G, S, cols, np.bincount(cols[1], minlength=G), seed=4)
    with w.ctx:
        w.expire("24 nodes: expire", [1])
        w.forget("24 nodes: forget", [int(w.tab.id[0])])
        w.surgery("the list grows", [(R, 0)] + [(A, i) for i in range(677)])
        assert w.N == 700 and w.tab.w
        w.forget("700 nodes: forget", [int(w.tab.id[-1])])
        w.expire("700 nodes: expire", [0, 2], deny=True)
        big = (rng.integers(0, 700, 900).astype(np.uint32), rng.integers(0, G, 900).astype(np.int32), rng.integers(0, 1000, (4 + S, 900)).astype(np.int64),
               rng.integers(0, 1 << S, 900).astype(np.uint32))
        big[3][big[0] >= 23] = 0                                               # (an appended node has no scalar keys: no row there claims one)
        w.ctx.wait_load(*big)                                                  # rows on the nodes beyond the old count
        w.tab = wr.load(700, G, S, *big)
        w.check("700 nodes: a table across all of them")
        w.expire("700 nodes: expire of every group", [4, 3, 2, 1, 0])
        assert w.tab.w == 0


# ---- lists from two bs_nodes_apply calls, equal counts, appends and updates only -----------------------------------------------------------
def _small(bsa, soa, orc, S=1, seed=11):
    N, G, rows = 9, 4, 50
    rng = np.random.default_rng(seed)
    cols = (rng.integers(0, N, rows).astype(np.uint32), rng.integers(0, G, rows).astype(np.int32), rng.integers(0, 1000, (4 + S, rows)).astype(np.int64),
            rng.integers(0, 1 << S, rows).astype(np.uint32))
    return table_ctx(bsa, soa, orc, N, G, S, cols, rng.integers(0, 30, G), seed=seed)


def test_two_node_patches_in_one_list_equal_counts_and_lists_that_move_nothing(bsa, soa, orc):
    w, reload = _small(bsa, soa, orc)
    ctx = w.ctx
    with ctx:
        e = w.surgery("two bs_nodes_apply calls, one list", [(R, 8), (A, 1), (R, 0), (A, 2), (R, 7), (U, 1), (R, 3)], split=3)
        assert e["n"] > 0 and w.N == 7
        reload()
        # ---- the count stays: the other calls were never refused, and the rows named other nodes
        before = w.tab.copy()
        kinds, idx = w.cut([(R, 0), (A, 1)])
        assert ctx.wait_count() == before.w and np.array_equal(ctx.wait_read()["node"], before.node), "equal count: the table passes the test of the counts"
        e = w.follow("the equal-count list", kinds, idx)
        keep = before.node != 0
        assert e["n"] == int((~keep).sum()) > 0 and w.N == 9
        assert not np.array_equal(w.tab.node, before.node[keep]), "the result differs from the untouched table"
        reload()
        # ---- APPENDs or UPDATEs only: the stale-count refusal is lifted and the rows are as they were
        before = w.tab.copy()
        kinds, idx = w.cut([(A, 1), (U, 2), (A, 3), (U, 10)])
        for fn in (ctx.wait_read, lambda: ctx.wait_release([0]), lambda: ctx.wait_expire([0]), lambda: ctx.wait_forget([0])):
            assert status_of(bsa, fn) == -4, "a stale node count"
        e = w.follow("appends and updates only", kinds, idx)
        assert e["n"] == 0 and w.N == 11 and all(np.array_equal(v, before.columns()[f]) for f, v in w.tab.columns().items())
        kinds, idx = w.cut([(U, 0), (U, 10)])
        assert w.follow("updates only", kinds, idx)["n"] == 0
        assert w.follow("an empty list with the counts in agreement", [], [])["n"] == 0
        kinds, idx = w.cut([(A, 0), (R, 11)])
        assert w.follow("an append that is removed again", kinds, idx)["n"] == 0 and w.N == 11
        w.expire("the table still expires", [0, 1, 2, 3], deny=True)


def test_caps_below_the_true_count_truncate_the_rows_only(bsa, soa, orc):
    w, reload = _small(bsa, soa, orc, S=0, seed=12)
    with w.ctx:
        for cap in (0, 2):
            e = w.surgery(f"cap {cap}", [(R, 4), (R, 4), (R, 0)], cap=cap)
            assert e["n"] > 2 and w.N == 6
            reload()
        n = C.c_uint32(77)
        kinds, idx = w.cut([(R, 8)])
        kv, iv = (C.c_uint32 * 1)(*kinds), (C.c_uint32 * 1)(*idx)
        exp = wn.nodes_apply(w.tab, w.st.matched, kinds, idx)
        assert w.ctx._lib.bs_wait_nodes_apply(w.ctx._h, 1, kv, iv, 0, None, None, None, C.byref(n)) == 0, "NULL result arrays with cap == 0"
        assert n.value == exp["n"] > 0
        w.check("cap 0 with NULL arrays")


# ---- errors: nothing resident changes --------------------------------------------------------------------------------------------------------
def test_every_refused_call_leaves_the_state_alone(bsa, soa, orc):
    u32a = lambda *v: (C.c_uint32 * max(len(v), 1))(*v)
    with bsa.Context(scalar_lanes=1, device=0) as fresh:
        assert status_of(bsa, lambda: fresh.wait_nodes_apply([], [], cap=0)) == -4, "no table, no nodes"
    with Case(bsa, soa, orc, waiting_scene(soa, [3, 2, 2], n_nodes=10, S=1, pods_cap=2, seed=43)) as c:
        ctx, lib = c.ctx, c.ctx._lib
        assert status_of(bsa, lambda: ctx.wait_nodes_apply([], [], cap=0)) == -4, "nodes and groups, no table"
        ctx.wait_load()
        w = WN(ctx, soa, orc, c.st, c.mg, wr.load(10, 3, 1), bn.NodeList(c.nodes, c.fit), c.pods, window=True)
        assert w.park("park")["n"] == 6 and sorted(set(w.tab.node.tolist())) == [0, 1, 2], "six pods wait on nodes 0, 1 and 2 (the last pod is rejected)"
        w.forget("one id dies", [2])
        n, out, gout = C.c_uint32(0), u32a(0, 0, 0, 0, 0, 0, 0, 0), (C.c_int32 * 8)()

        def raw(count, kind, index, cap=0, id_=None, node=None, group=None, n_out=C.byref(n)):
            return lambda: ctx._chk(lib.bs_wait_nodes_apply(ctx._h, count, kind, index, cap, id_, node, group, n_out), "bs_wait_nodes_apply")
        call = lambda kinds, idx: (lambda: ctx.wait_nodes_apply(kinds, idx))
        refused = [("a kind outside the three", -1, call([3], [0])), ("UPDATE at the count", -1, call([U], [10])), ("REMOVE at the count", -1, call([R], [10])),
                   ("the eleventh REMOVE of ten nodes", -1, call([R] * 11, [0] * 11)), ("UPDATE beyond an APPEND", -1, call([A, U], [0, 11])),
                   ("a bad delta behind good ones", -1, call([R, A, U, 7], [1, 0, 9, 0])),
                   ("NULL kind", -1, raw(1, None, u32a(0))), ("NULL index", -1, raw(1, u32a(U), None)),
                   ("NULL id with a cap", -1, raw(1, u32a(U), u32a(0), 8, None, out, gout)), ("NULL node with a cap", -1, raw(1, u32a(U), u32a(0), 8, out, None, gout)),
                   ("NULL group with a cap", -1, raw(1, u32a(U), u32a(0), 8, out, out, None)), ("NULL n_out", -1, raw(1, u32a(U), u32a(0), n_out=None))]
        # ---- the counts agree: a list that ends elsewhere is not the list bs_nodes_apply got
        for where, want, fn in refused + [("a REMOVE bs_nodes_apply never saw", -4, call([R], [0])), ("an APPEND it never saw", -4, call([A], [0]))]:
            assert status_of(bsa, fn) == want, where
            w.check(f"after the refused call: {where}")
        ctx.set_shard(0, 2)
        assert status_of(bsa, lambda: ctx.wait_nodes_apply([], [], cap=0)) == -4, "a sharded context"
        ctx.set_shard(0, 1)
        w.check("after the sharded call")
        ids, old, grp, k = ctx.wait_nodes_apply([], [])
        assert k == 0 and ids.size == 0
        w.check("count == 0 with the counts in agreement")
        # ---- a stale node count: the other calls answer BS_ERR_STATE before and after every refused call
        kinds, idx = w.cut([(R, 1)])

        def stale(where):
            assert (ctx.wait_count(), ctx.wait_ids()) == (w.tab.w, w.tab.ids), where
            for fn in (ctx.wait_read, lambda: ctx.wait_release([0]), lambda: ctx.wait_expire([0]), lambda: ctx.wait_forget([0]), ctx.wait_park):
                assert status_of(bsa, fn) == -4, f"{where}: a stale node count"
            req, pres = ctx.read_node_requests()
            assert np.array_equal(req, w.st.requested) and np.array_equal(pres, w.st.requested_present), f"{where}: node requests"
            w.mg.matched[:], w.mg.flags[:] = w.st.matched, w.st.flags
            assert_groups_equal(ctx.read_groups(), w.mg, soa, where)
        stale("after the surgery")
        for where, want, fn in refused[:1] + [("REMOVE at the table's count", -1, call([R], [10])), ("an empty list with stale counts", -4, call([], [])),
                                              ("two REMOVEs where one happened", -4, call([R, R], [1, 1]))] + refused[6:]:
            assert status_of(bsa, fn) == want, where
            stale(f"after the refused call: {where}")
        ctx.set_shard(0, 2)
        assert status_of(bsa, lambda: ctx.wait_nodes_apply(kinds, idx, cap=0)) == -4, "a sharded context"
        ctx.set_shard(0, 1)
        stale("after the sharded call")
        e = w.follow("the list bs_nodes_apply got", kinds, idx)          # (the model's table is the one from before the refused calls)
        assert e["n"] == 1 and w.N == 9, "node 1 held ids 2 and 3; id 2 died above"
        # ---- a stale group count
        bigger = soa.Groups.empty(4, c.nodes.lanes)
        bigger.min_member[:] = 9
        ctx.load_groups(bigger)
        assert status_of(bsa, lambda: ctx.wait_nodes_apply([], [], cap=0)) == -4, "a stale group count"
        assert (ctx.wait_count(), ctx.wait_ids()) == (w.tab.w, w.tab.ids)
        w.mg.matched[:], w.mg.flags[:] = w.st.matched, w.st.flags
        ctx.load_groups(w.mg)
        w.check("the group count is back")
        w.expire("and the state still expires", [0, 1, 2], deny=True)
        assert w.tab.w == 0


# ---- down to zero nodes and back -------------------------------------------------------------------------------------------------------------
def test_down_to_zero_nodes_and_back(bsa, soa, orc):
    scene = waiting_scene(soa, [3, 2], n_nodes=8, S=1, pods_cap=2, matched0=[1, 0], seed=44)
    rng = np.random.default_rng(45)
    with Case(bsa, soa, orc, scene) as c:
        ctx = c.ctx
        ctx.wait_load()
        w = WN(ctx, soa, orc, c.st, c.mg, wr.load(8, 2, 1), bn.NodeList(c.nodes, c.fit), c.pods, window=True)
        assert w.park("park")["n"] == 3 and sorted(set(w.tab.node.tolist())) == [0, 1], "three pods wait, on two nodes (the second gang is rejected)"
        e = w.surgery("every node leaves", remove_steps(rng, range(8)))
        assert e["n"] == 3 and w.tab.w == 0 and w.N == 0 and ctx.n == 0 and w.st.matched.tolist() == [1, 0]
        assert w.surgery("nothing on nothing", [])["n"] == 0
        e = w.surgery("eight nodes are appended", [(A, i) for i in range(8)])
        assert e["n"] == 0 and w.N == 8
        w.run_pass("a pass on the new list", c.pods, c.s["leader"])
        pk = w.park("park again")
        assert pk["n"] == 3 and pk["first_id"] == 3, "the table works again from empty; the dropped ids stay dead"
        assert status_of(bsa, lambda: ctx.wait_forget([0])) == -1, "a dropped id is dead"
        w.check("after the dead id")
        assert w.expire("expire", [1, 0], deny=True)["n"] == 3 and w.tab.w == 0
