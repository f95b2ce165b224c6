"""GPU tests of bs_nominated_nodes_apply (csrc/bs_nominated.hpp: k_nn_move<S>, then k_nm_chains for the new node count): after
bs_nodes_apply + bs_nominated_nodes_apply the resident nominated-pod table, its ids and the returned rows equal the array model of
tests/nominated_nodes_ref.py, and the three preemption calls answer as a twin context that loaded the new node list and the model's rows
afresh — and as tests/nominated_ref.py's reference on the remapped scene (tests/nominated_nodes_scenes.World keeps that scene).  The seeds
are verified on the model by tests/test_nominated_nodes_cpu.py.  All comparisons are bit-exact.  The shapes are small: 24 to 96 nodes (700
once, for chain heads beyond the old count), at most 24 preemptors, tables of at most 2049 rows (1023 / 1024 / 1025 / 2049: the
compaction's window edge)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import nominated_nodes_ref as nn
import nominated_nodes_scenes as ns
import nominated_ref as nr
import test_gpu_nominated as tg
from preempt_scenes import groups_for

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
U, A, R = nn.UPDATE, nn.APPEND, nn.REMOVE
INVALID, STATE_ERR = -1, -4
MODES = ns.MODES
STATE = ("req", "pres", "bound_id", "bound_node")


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _ctx(w: ns.World, bound=True, table=True):
    """a context that holds what the world holds now"""
    sc = w.scene()
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    if bound:
        ctx.load_bound(sc["bound"])
        ctx.bound_pdb_set(sc["violating"])
    if table and w.tab.loaded:
        r = w.rows()
        ctx.nominated_load(r["node"], r["priority"], r["req"], r["req_present"])
    return ctx


def _surgery(ctx, w, steps, where, cap=None, bound=True, first="bound", split=()):
    """bs_nodes_apply of steps (in one call, or cut at `split`), then the two remaps in the order asked; the dropped rows and the table
    against the model.  -> the model's dropped rows"""
    ids0 = ctx.nominated_ids()
    deltas, kinds, idx = w.cut(steps)
    cuts = [0, *split, len(deltas)]
    for a, b in zip(cuts, cuts[1:]):
        if b > a:
            ctx.apply_node_deltas(deltas[a:b])
    assert ctx.n == w.nl.n
    exp = w.follow(kinds, idx)
    if bound and first == "bound":
        ctx.bound_nodes_apply(kinds, idx)
    ids, old, prio, n = ctx.nominated_nodes_apply(kinds, idx, cap=cap)
    if bound and first != "bound":
        ctx.bound_nodes_apply(kinds, idx)
    k = exp["n"] if cap is None else min(exp["n"], cap)
    assert n == exp["n"], f"{where}: n {n}, the model drops {exp['n']}"
    assert np.array_equal(ids, exp["id"][:k]) and np.array_equal(old, exp["node"][:k]) and np.array_equal(prio, exp["priority"][:k]), f"{where}: the dropped rows"
    tg._read_equal(ctx, w.rows(), where)
    assert ctx.nominated_ids() == ids0 == w.tab.ids, f"{where}: bs_nominated_ids is unchanged"
    return exp


def _answers(ctx, w, where, twin=None, modes=MODES):
    """the three calls (no APPLY) against the reference on the world as it is now, and against a twin context"""
    sc = w.scene()
    for mode in modes:
        got = tg._call(ctx, mode, sc)
        exp = w.mapped(w.expect_raw(mode))
        tg._same(got, exp["res"], f"{where}: {mode} against the reference")
        if mode == "gang":
            tg._same(got, exp, f"{where}: gang", ("slot_voided", "group_placed"))
        if twin is not None:
            want = tg._call(twin, mode, sc)
            want["victims"] = w.mapped(dict(res=want))["res"]["victims"]       # (the twin's ids are indices of the world's bound table)
            tg._same(got, want, f"{where}: {mode} against the twin")
            if mode == "gang":
                tg._same(got, want, f"{where}: gang against the twin", ("slot_voided", "group_placed"))


def _plain_world(n, rows, S=1, seed=51, node=None):
    """a small scene on n nodes with a table of `rows` rows drawn from the queue's pods"""
    sc = ns.base_scene(seed, S, False, n=n, q=12)
    rng = np.random.default_rng(rows * 7 + n)
    src = rng.integers(0, sc["pods"].p, size=rows)
    node = rng.integers(0, n, size=rows) if node is None else node
    t = tg._table(sc, node, rng.integers(0, 6000, size=rows), sc["pods"].req[: 4 + S, src], sc["pods"].req_present[src])
    return ns.World(sc, t)


# ---- 1. the hand known answers ---------------------------------------------------------------------------------------------------------
def test_hand_known_answers_on_device():
    for case in nn.hand_kats():
        sc = ns.base_scene(7, 0, False, n=case["n"], q=4)
        w = ns.World(sc, nn.kat_table(case).read())
        e = case["expect"]
        with _ctx(w, bound=False) as ctx:
            steps = [(k, 0 if k == A else i) for k, i in zip(case["kind"], case["index"])]
            out = _surgery(ctx, w, steps, case["name"], bound=False)
            got = ctx.nominated_read()
            assert ctx.n == e["n_new"] and out["n"] == len(e["dropped"]["id"]), case["name"]
            assert (got["id"].tolist(), got["node"].tolist(), got["priority"].tolist()) == (e["table_id"], e["table_node"], e["table_priority"]), case["name"]
            assert out["id"].tolist() == e["dropped"]["id"] and out["node"].tolist() == e["dropped"]["node"], case["name"]


# ---- 2. remap equals fresh load ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sorted(ns.TWIN_SEEDS))
def test_the_remap_equals_a_fresh_load_and_the_reference(S):
    w, steps = ns.twin_scene(S)
    with _ctx(w) as ctx:
        out = _surgery(ctx, w, steps, f"S={S}")
        assert out["n"] >= 1
        with _ctx(w) as twin:                                # the new node list, the surviving bound pods, the model's rows: all loaded afresh
            a, b = ctx.nominated_read(), twin.nominated_read()
            for f in ("node", "priority", "req", "req_present"):
                assert np.array_equal(a[f], b[f]), f"S={S}: column {f} against the fresh load"
            assert np.array_equal(a["id"], w.tab.id)
            _answers(ctx, w, f"S={S}", twin)
        bare = w.expect_raw("commit", rows=None)["res"]
        assert nr.changed(w.expect_raw("commit")["res"], bare), "the surviving rows change no answer"


# ---- 3. appends only ------------------------------------------------------------------------------------------------------------------------
def test_appends_only_makes_heads_for_the_new_count():
    """24 -> 700 nodes: no row moves, but the victim search reads one chain head per node.  Then rows on nodes beyond the old count, which
    the next calls count (the CPU test asserts that these rows change an answer)"""
    w, steps, rows_for = ns.appends_scene()
    rows = w.rows()
    with _ctx(w) as ctx:
        out = _surgery(ctx, w, steps, "appends only")
        assert out["n"] == 0 and ctx.n == 700 and np.array_equal(w.rows()["node"], rows["node"])
        with _ctx(w) as twin:
            _answers(ctx, w, "24 -> 700", twin)
            args = rows_for(w)
            assert min(args[2]) >= 24
            assert ctx.nominated_apply(*args) == w.tab.apply(*args, w.sc["pods"]) == twin.nominated_apply(*args)
            tg._read_equal(ctx, w.rows(), "rows beyond the old count")
            _answers(ctx, w, "with rows on appended nodes", twin)


# ---- 4. a remove and an append in one batch -----------------------------------------------------------------------------------------------------
def test_surgery_that_keeps_the_count_is_put_right():
    w, _ = ns.twin_scene(2)
    stale = w.rows()
    holder = int(np.unique(stale["node"])[0])
    with _ctx(w) as ctx:
        deltas, kinds, idx = w.cut([(R, holder), (A, 3)])
        ctx.apply_node_deltas(deltas)
        ctx.bound_nodes_apply(kinds, idx)
        assert ctx.n == 48, "the count is kept: the stale test of the other calls passes"
        # on the model: without the call the rows sit on the wrong nodes, and the answers show it
        moved = nn.remap_on_the_host(stale, 48, kinds, idx, 2)
        assert any(nr.changed(w.expect_raw(m, rows=moved)["res"], w.expect_raw(m, rows=stale)["res"]) for m in MODES)
        got = tg._call(ctx, "run", w.scene())                # legal, and wrong: the hazard the call closes
        tg._same(got, w.mapped(w.expect_raw("run", rows=stale))["res"], "before the call: the stale rows, as they are")
        exp = w.follow(kinds, idx)
        ids, old, prio, n = ctx.nominated_nodes_apply(kinds, idx)
        assert n == exp["n"] >= 1 and np.array_equal(ids, exp["id"]) and np.all(old == holder)
        tg._read_equal(ctx, w.rows(), "equal count")
        with _ctx(w) as twin:
            _answers(ctx, w, "equal count", twin)


# ---- 5. window edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1023, 1024, 1025, 2049])
def test_drops_across_the_compaction_window_edges(m):
    """node 0 holds the first row, node 1 the last, nodes 2 and 3 the rows on both sides of each 1024 boundary; they leave one list after
    the other, then nothing, then everything"""
    n = 40
    rng = np.random.default_rng(m)
    node = rng.integers(4, n, size=m)
    for edge in range(1024, m, 1024):
        node[edge - 1], node[edge] = 2, 3
    node[0], node[m - 1] = 0, 1                             # (1025 rows: the last row IS the row behind the boundary)
    w = _plain_world(n, m, node=node)
    with _ctx(w, bound=False) as ctx:
        first = _surgery(ctx, w, [(R, 0)], f"m={m}: the first row", bound=False)
        assert first["id"].tolist() == [0]
        last = _surgery(ctx, w, [(R, 0)], f"m={m}: the last row", bound=False)                  # old node 1 is index 0 now
        assert last["id"].tolist() == [m - 1]
        if m > 1024:
            edges = _surgery(ctx, w, [(R, 1), (R, 0), (A, 5)], f"m={m}: both sides of each boundary", bound=False)
            assert edges["id"].tolist() == np.nonzero(np.isin(node, [2, 3]))[0].tolist() and edges["n"] >= 1
        none = _surgery(ctx, w, [(A, 1), (U, 3), (R, w.nl.n)], f"m={m}: none", bound=False)
        assert none["n"] == 0
        many = _surgery(ctx, w, ns.remove_steps(rng, range(5, 25)), f"m={m}: twenty nodes", bound=False, cap=7)
        assert many["n"] > 300
        left = w.tab.id.size
        rest = _surgery(ctx, w, ns.remove_steps(rng, range(w.nl.n)), f"m={m}: all rows", bound=False)
        assert rest["n"] == left > 0 and ctx.nominated_count() == 0 and ctx.nominated_ids() == m and ctx.n == 0


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------------
def test_empty_tables_zero_nodes_updates_only_and_a_list_from_three_calls():
    w = _plain_world(24, 0)
    with _ctx(w, bound=False) as ctx:                        # from an empty table
        assert _surgery(ctx, w, [(R, 3), (A, 1), (A, 2)], "an empty table", bound=False)["n"] == 0 and ctx.n == 25
        args = ([], [1, 2, 3], [24, 0, 5], [9, 8, 7])
        assert ctx.nominated_apply(*args) == w.tab.apply(*args, w.sc["pods"]) == 0
        assert _surgery(ctx, w, [(U, 0), (U, 24)], "UPDATEs only", bound=False)["n"] == 0
        out = _surgery(ctx, w, [(R, 24), (R, 0), (R, 4)], "down to an empty table", bound=False)          # old nodes 24, 0 and 5 (index 4 by then)
        assert out["id"].tolist() == [0, 1, 2] and out["node"].tolist() == [24, 0, 5] and ctx.nominated_count() == 0
    w = _plain_world(24, 30, S=0)
    rng = np.random.default_rng(3)
    with _ctx(w, bound=False) as ctx:
        out = _surgery(ctx, w, ns.remove_steps(rng, range(24)), "down to zero nodes", bound=False)
        assert out["n"] == 30 and ctx.n == 0 and ctx.nominated_count() == 0 and ctx.nominated_ids() == 30
        assert _surgery(ctx, w, [], "nothing on nothing", bound=False)["n"] == 0
        assert _surgery(ctx, w, [(A, i) for i in range(24)], "and back", bound=False)["n"] == 0 and ctx.n == 24
        assert ctx.nominated_apply([], [0], [23], [1]) == w.tab.apply([], [0], [23], [1], w.sc["pods"]) == 30
        tg._read_equal(ctx, w.rows(), "the table works again from empty")
    w = _plain_world(24, 60, S=2)
    with _ctx(w) as ctx:                                     # three bs_nodes_apply calls, one list, with a cancelled append in it
        out = _surgery(ctx, w, [(R, 5), (A, 1), (R, 23), (U, 2), (R, 0), (A, 7), (R, 10)], "three calls", split=(2, 4))
        assert out["n"] >= 3 and ctx.n == 22
        _answers(ctx, w, "three calls", modes=("run",))


# ---- 7. cap ------------------------------------------------------------------------------------------------------------------------------
def test_caps_below_the_true_count_truncate_the_rows_only():
    for cap in (0, 2):
        w = _plain_world(24, 200)
        with _ctx(w) as ctx:
            out = _surgery(ctx, w, [(R, 4), (R, 4), (R, 0)], f"cap {cap}", cap=cap)
            assert out["n"] > 2
            _answers(ctx, w, f"cap {cap}", modes=("run",))
    w = _plain_world(24, 200)
    with _ctx(w, bound=False) as ctx:
        deltas, kinds, idx = w.cut([(R, 8)])
        ctx.apply_node_deltas(deltas)
        exp = w.follow(kinds, idx)
        n = C.c_uint32(77)
        kv, iv = (C.c_uint32 * 1)(*kinds), (C.c_uint32 * 1)(*idx)
        assert ctx._lib.bs_nominated_nodes_apply(ctx._h, 1, kv, iv, 0, None, None, None, C.byref(n)) == 0, "NULL result arrays with cap == 0"
        assert n.value == exp["n"] > 0
        tg._read_equal(ctx, w.rows(), "cap 0 with NULL arrays")


# ---- 8. ids ------------------------------------------------------------------------------------------------------------------------------
def test_ids_survive_dropped_ids_are_dead_and_nominee_ids_still_name_their_rows():
    w = ns.World(ns.base_scene(71, 2, False, n=24, q=12))
    w.tab.load(24, [], [], np.zeros((6, 0)), [])
    with _ctx(w) as ctx:
        sc = w.scene()
        got = tg._call(ctx, "commit", sc, apply=True, nominate=True)
        raw = w.expect_raw("commit", True, False)
        tg._same(got, w.mapped(raw)["res"], "the first commit")
        ids = w.nominate(raw)
        w.applied(raw)
        assert np.array_equal(got["nominated_id"], ids) and int((ids != nr.NONE).sum()) >= 3
        held = w.rows()
        gone_node = int(held["node"].min())                    # the lowest node that holds a nominee: every other nominee's node moves down
        out = _surgery(ctx, w, [(R, gone_node), (A, 2)], "a nominee's node leaves", first="nominated")
        assert 1 <= out["n"] < held["id"].size
        assert ctx.nominated_ids() == held["id"].size
        live = ctx.nominated_read()
        for i in np.nonzero(ids != nr.NONE)[0]:                # the ids bs_preempt_nominated_read handed out still name their rows
            at = np.nonzero(live["id"] == ids[i])[0]
            if int(ids[i]) in out["id"].tolist():
                assert at.size == 0
            else:
                assert at.size == 1 and int(live["priority"][at[0]]) == int(sc["priority"][i])
                assert np.array_equal(live["req"][:3, at[0]], sc["pods"].req[:3, int(sc["pod_index"][i])])
        assert np.array_equal(ctx.preempt_nominated_read(12), ids)
        tg._refused(INVALID, ctx.nominated_apply, [int(out["id"][0])])
        tg._read_equal(ctx, w.rows(), "after naming a dropped id")
        first = ctx.nominated_apply([], [0], [1], [5])
        assert first == w.tab.apply([], [0], [1], [5], sc["pods"]) == held["id"].size, "the next insert starts at bs_nominated_ids"
        survivor = int(w.tab.id[0])
        ctx.nominated_apply([survivor])
        w.tab.apply([survivor], [], [], [], sc["pods"])
        tg._read_equal(ctx, w.rows(), "a survivor's id still removes its row")


# ---- 9. a twin that outgrows its headroom between two calls ------------------------------------------------------------------------------------
def test_rows_then_nodes_outgrow_the_twin():
    w = _plain_world(24, 40, S=2)
    rng = np.random.default_rng(9)
    with _ctx(w) as ctx:
        _surgery(ctx, w, [(R, 2)], "a first remap: both allocations exist")
        for ni in (300, 900):                                # a small load leaves room for 256 rows: both inserts outgrow their allocation
            args = ([], rng.integers(0, w.sc["pods"].p, size=ni), rng.integers(0, w.nl.n, size=ni), rng.integers(0, 6000, size=ni))
            assert ctx.nominated_apply(*args) == w.tab.apply(*args, w.sc["pods"])
        out = _surgery(ctx, w, [(A, i % 24) for i in range(300)] + [(R, 1), (R, 7)], "rows grew, then the node count")
        assert out["n"] > 20 and ctx.n == 321
        _answers(ctx, w, "after growing", modes=("run", "commit"))
        out = _surgery(ctx, w, [(R, 0)] * 280, "and down again")
        assert ctx.n == 41 and out["n"] > 100
        _answers(ctx, w, "after shrinking", modes=("run",))


# ---- 10. a real cycle ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["bound", "nominated"])
def test_a_cycle_commit_surgery_both_remaps_commit(first):
    """commit(APPLY | NOMINATE) -> surgery that removes a node holding a nominee and one holding none -> both remaps, in either order ->
    commit again.  Results, applied state and table equal the reference on the remapped scene"""
    sc = ns.base_scene(81, 2, False, n=24, q=24)
    half = np.arange(24) < 12
    w = ns.World(sc)
    w.tab.load(24, [], [], np.zeros((6, 0)), [])
    with _ctx(w) as ctx:
        got = tg._call(ctx, "commit", dict(sc, pod_index=sc["pod_index"][half], priority=sc["priority"][half]), apply=True, nominate=True)
        raw = w.expect_raw("commit", True, False, pick=half)
        exp = w.mapped(raw)
        tg._same(got, exp["res"], "cycle 1")
        ids = w.nominate(raw, pick=half)
        w.applied(raw)
        assert np.array_equal(got["nominated_id"], ids)
        tg._same(tg._state(ctx), exp, "cycle 1 state", STATE)
        held = np.unique(w.tab.node)
        free = np.setdiff1d(np.arange(24), held)
        assert held.size >= 2 and free.size >= 1
        out = _surgery(ctx, w, ns.remove_steps(np.random.default_rng(1), [int(held[0]), int(free[0])]) + [(A, 4)], "the surgery", first=first)
        assert 1 <= out["n"] < int((ids != nr.NONE).sum()) and ctx.n == 23
        got2 = tg._call(ctx, "commit", dict(sc, pod_index=sc["pod_index"][~half], priority=sc["priority"][~half]), apply=True, nominate=True)
        raw2 = w.expect_raw("commit", True, False, pick=~half)
        exp2 = w.mapped(raw2)
        tg._same(got2, exp2["res"], "cycle 2")
        ids2 = w.nominate(raw2, pick=~half)
        w.applied(raw2)
        assert np.array_equal(got2["nominated_id"], ids2)
        tg._same(tg._state(ctx), exp2, "cycle 2 state", STATE)
        tg._read_equal(ctx, w.rows(), "cycle 2 rows")


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refused_call_changes_nothing():
    u32a = lambda *v: (C.c_uint32 * max(len(v), 1))(*v)
    w = _plain_world(24, 50, S=2)
    with bsa.Context(scalar_lanes=2, device=0) as fresh:
        tg._refused(STATE_ERR, fresh.nominated_nodes_apply, [], [], cap=0)               # no table, no nodes
        fresh.load_nodes(w.sc["nodes"], w.sc["fit"])
        tg._refused(STATE_ERR, fresh.nominated_nodes_apply, [], [], cap=0)               # nodes, no table
    with _ctx(w) as ctx:
        lib = ctx._lib
        ctx.nominated_apply([1, 2])
        w.tab.apply([1, 2], [], [], [], w.sc["pods"])
        n, out, pout = C.c_uint32(0), u32a(*([0] * 8)), (C.c_int32 * 8)()

        def raw(count, kind, index, cap=0, id_=None, node=None, prio=None, n_out=C.byref(n)):
            return lambda: ctx._chk(lib.bs_nominated_nodes_apply(ctx._h, count, kind, index, cap, id_, node, prio, n_out), "bs_nominated_nodes_apply")
        call = lambda kinds, idx: (lambda: ctx.nominated_nodes_apply(kinds, idx))
        refused = [("a kind outside the three", INVALID, call([3], [0])), ("UPDATE at the count", INVALID, call([U], [24])),
                   ("REMOVE at the count", INVALID, call([R], [24])), ("the 25th REMOVE of 24 nodes", INVALID, call([R] * 25, [0] * 25)),
                   ("UPDATE beyond an APPEND", INVALID, call([A, U], [0, 25])), ("a bad delta behind good ones", INVALID, call([R, A, U, 7], [1, 0, 9, 0])),
                   ("NULL kind", INVALID, raw(1, None, u32a(0))), ("NULL index", INVALID, raw(1, u32a(U), None)),
                   ("NULL id with a cap", INVALID, raw(1, u32a(U), u32a(0), 8, None, out, pout)),
                   ("NULL node with a cap", INVALID, raw(1, u32a(U), u32a(0), 8, out, None, pout)),
                   ("NULL priority with a cap", INVALID, raw(1, u32a(U), u32a(0), 8, out, out, None)),
                   ("NULL n_out", INVALID, raw(1, u32a(U), u32a(0), n_out=None))]
        before = (tg._state(ctx), ctx.bound_dump())

        def unchanged(where, stale=False):
            assert (ctx.nominated_count(), ctx.nominated_ids()) == (w.tab.id.size, w.tab.ids), where
            if stale:
                tg._refused(STATE_ERR, ctx.nominated_read)
            else:
                tg._read_equal(ctx, w.rows(), where)
            st, dump = tg._state(ctx), ctx.bound_dump()
            assert all(np.array_equal(st[f], before[0][f]) for f in st) and all(np.array_equal(dump[f], before[1][f]) for f in dump), where
        for where, want, fn in refused + [("a REMOVE bs_nodes_apply never saw", STATE_ERR, call([R], [0])), ("an APPEND it never saw", STATE_ERR, call([A], [0]))]:
            tg._refused(want, fn)
            unchanged(where)
        ctx.set_shard(0, 2)
        tg._refused(STATE_ERR, ctx.nominated_nodes_apply, [], [], cap=0)                 # a sharded context
        ctx.set_shard(0, 1)
        ctx.reduce_external(True)
        tg._refused(STATE_ERR, ctx.nominated_nodes_apply, [], [], cap=0)                 # an external-reduce context
        ctx.reduce_external(False)
        unchanged("after the sharded calls")
        ids, old, prio, k = ctx.nominated_nodes_apply([], [])
        assert k == 0 and ids.size == 0
        unchanged("count == 0 with the counts in agreement")
        # ---- a stale node count: every refused call leaves the table stale and whole
        deltas, kinds, idx = w.cut([(R, 1)])
        ctx.apply_node_deltas(deltas)
        ctx.bound_nodes_apply(kinds, idx)
        before = (tg._state(ctx), ctx.bound_dump())
        for where, want, fn in refused[:1] + [("REMOVE at the table's count", INVALID, call([R], [24])), ("an empty list with stale counts", STATE_ERR, call([], [])),
                                              ("two REMOVEs where one happened", STATE_ERR, call([R, R], [1, 1]))] + refused[6:]:
            tg._refused(want, fn)
            unchanged(f"stale: {where}", stale=True)
            tg._refused(STATE_ERR, tg._call, ctx, "run", w.scene())
        exp = w.follow(kinds, idx)
        ids, old, prio, k = ctx.nominated_nodes_apply(kinds, idx)
        assert k == exp["n"] and np.array_equal(ids, exp["id"])
        unchanged("the list bs_nodes_apply got")
        _answers(ctx, w, "after the refusals", modes=("run",))


# ---- 12. random steps against the model ---------------------------------------------------------------------------------------------------------
def test_twenty_seeds_of_twelve_random_steps():
    drops, kinds = 0, dict.fromkeys(ns.FUZZ_KINDS, 0)
    for seed in ns.FUZZ_SEEDS:
        run = ns.fuzz_run(seed)
        _, w, rows = next(run)
        sc0 = w.scene()
        ctx = bsa.Context(scalar_lanes=sc0["S"], device=0)
        with ctx:
            ctx.load_nodes(sc0["nodes"], sc0["fit"])
            ctx.load_groups(groups_for(sc0))
            ctx.load_pods(sc0["pods"])
            ctx.load_bound(sc0["bound"])
            ctx.bound_pdb_set(sc0["violating"])
            ctx.nominated_load(rows["node"], rows["priority"], rows["req"], rows["req_present"])
            for step, item in enumerate(run):
                where = f"seed {seed} step {step} {item[0]}"
                kinds[item[0]] += 1
                if item[0] == "apply":
                    assert ctx.nominated_apply(*item[1]) == item[2], where
                elif item[0] == "surgery":
                    _, deltas, kv, iv, exp = item
                    ctx.apply_node_deltas(deltas)
                    if step & 1:
                        ctx.bound_nodes_apply(kv, iv)
                    ids, old, prio, n = ctx.nominated_nodes_apply(kv, iv)
                    if not step & 1:
                        ctx.bound_nodes_apply(kv, iv)
                    assert n == exp["n"] and np.array_equal(ids, exp["id"]) and np.array_equal(old, exp["node"]) and np.array_equal(prio, exp["priority"]), where
                    drops += n
                elif item[0] == "call":
                    got = tg._call(ctx, item[1], w.sc)
                    tg._same(got, item[2]["res"], where)
                else:
                    got = tg._call(ctx, item[1], w.sc, apply=True, nominate=True)
                    tg._same(got, item[2]["res"], where)
                    assert np.array_equal(got["nominated_id"], item[3]), where
                    tg._same(tg._state(ctx), item[2], where + " state", STATE)
                    if item[1] == "gang":
                        tg._same(got, item[2], where, ("slot_voided", "group_placed"))
                tg._read_equal(ctx, w.rows(), where)
                assert ctx.nominated_ids() == w.tab.ids and ctx.n == w.nl.n, where
    assert drops >= 20 and all(kinds.values()), (drops, kinds)
