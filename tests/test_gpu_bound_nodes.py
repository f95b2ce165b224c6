"""GPU tests of bs_bound_nodes_apply: after bs_nodes_apply + bs_bound_nodes_apply the resident bound table equals the numpy model of
tests/bound_nodes_ref.py (every column, the PDB bits, the dropped ids in the old table's order) and equals a second context that LOADED
the post-surgery node list and the surviving entries, in what bs_preempt_run and bs_preempt_commit(APPLY) answer on it, victims mapped
through the monotone id map.  Shapes are the smallest at which each piece can go wrong: node counts around one wave, the move's four
nodes per workgroup, the 256-thread blocks and the scan's 1024-entry blocks (two blocks and the prefix launch at 1025); per-node lengths
around the 64-entry copy step; no scalar lanes and two."""
import ctypes
import importlib

import numpy as np
import pytest

import bound_apply_ref as ba
import bound_nodes_ref as bn
import preempt_pdb_ref as pp
from preempt_scenes import groups_for
from test_gpu_bound_apply import CAP, _check_table, _compare, _evict, _map, _same_state, _scene, _state, _take, _trim, _ungrouped_pool

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth = bsa.soa, bsa.synth
U, A, R = bn.UPDATE, bn.APPEND, bn.REMOVE
LENS = [0, 1, 63, 64, 65, 130]


def _ctx(sc, nodes, fit, bound, bits=None):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(nodes, fit)
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(bound)
    if bits is not None:
        ctx.bound_pdb_set(bits)
    return ctx


def _lens_scene(seed, counts, S, groups=0):
    """a scene whose node k holds exactly counts[k] bound pods"""
    sc, bits = _scene(seed, len(counts), 130, S, groups=groups)
    sc = _trim(sc, counts)
    assert np.bincount(sc["bound"].node, minlength=len(counts)).tolist() == list(counts)
    return sc, bits[: sc["bound"].b]


def _surgery(ctx, nl, t, steps, dropped_cap=None, where=""):
    """steps = [(kind, index)]: the node list, the mirror and the model follow them; the device's dropped ids against the model's.
    dropped_cap None = room for every entry.  Returns the dropped ids."""
    req, pres = ctx.read_node_requests()                    # (the node requests as the device holds them: an UPDATE sends them again)
    nl.req, nl.rpres = np.array(req, np.int64), np.array(pres, np.uint32)
    deltas = [nl.append(int(i) % len(nl.pool[1])) if k == A else nl.remove(int(i)) if k == R else nl.update(int(i)) for k, i in steps]
    ctx.apply_node_deltas(deltas)
    assert ctx.n == nl.n
    kinds, idx = [d.kind for d in deltas], [d.index for d in deltas]
    cap = t.count if dropped_cap is None else dropped_cap
    nd, ids = ctx.bound_nodes_apply(kinds, idx, cap)
    _, dropped, n2 = bn.nodes_apply(t, kinds, idx, n_expected=nl.n)
    assert nd == dropped.size, f"{where}: n_dropped {nd}, the model drops {dropped.size}"
    assert np.array_equal(ids, dropped[:cap]), f"{where}: dropped ids {ids[:20]} vs {dropped[:20]} (cap {cap})"
    _check_table(ctx, t, where)
    return dropped


def _check_vs_load(sc, nl, ctx, t, where, commit=True, sel=slice(None)):
    """a second context loads the post-surgery node list (with the followed context's node requests) and the surviving entries: same
    table through the id map, same answers of preempt() and, with commit, of preempt_commit(apply=True), same table after it"""
    eq, keep, bits = t.equivalent()
    req, pres = ctx.read_node_requests()
    pi, pr = sc["pod_index"][sel], sc["priority"][sel]
    with _ctx(sc, nl.nodes(req, pres), nl.fit(), eq, bits) as ref:
        def same_table(what):
            ids_a, nodes_a = ctx.read_bound()
            ids_b, nodes_b = ref.read_bound()
            assert np.array_equal(keep[ids_b] if keep.size else ids_b, ids_a) and np.array_equal(nodes_a, nodes_b), f"{where}: table {what}"
            da, db = ctx.bound_dump(), ref.bound_dump()
            for f in ba.COLUMNS:
                assert np.array_equal(da[f], db[f]), f"{where}: column {f} {what}"
        same_table("vs the load")
        got = ctx.preempt(pi, pr, sc["protected"], victim_cap=CAP)
        _compare(got, _map(ref.preempt(pi, pr, sc["protected"], victim_cap=CAP), keep), f"{where}: preempt vs the load")
        if not commit:
            return got
        got = ctx.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP, apply=True)
        assert got["n_victims"].max(initial=0) <= CAP
        _compare(got, _map(ref.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP, apply=True), keep), f"{where}: commit vs the load")
        ra, rb = ctx.read_node_requests(), ref.read_node_requests()
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), f"{where}: node requests after the commit"
        same_table("after the commit")
    return got


def _steps(rng, n, kind):
    """a delta list of one kind on a list of n nodes; never down to zero nodes"""
    if kind == "equal":                                     # the count stays
        return [(R, 0), (A, rng.integers(0, 99))]
    if kind == "grow":
        return [(U, rng.integers(0, n)), (A, 1), (A, 2), (U, n + 1)]
    if kind == "shrink":                                    # the last, then two in the middle by the same index, one append to stay above zero
        out = [(A, 3), (R, n - 1)]
        if n >= 3:
            out += [(R, n // 2), (R, n // 2)]
        return out
    if kind == "cancel":
        return [(A, 4), (R, rng.integers(0, n)), (A, 5), (R, n), (U, n - 1)]
    if kind == "many":                                      # a quarter of the nodes, random current indices, updates in between
        out, cur = [(A, 6)], n + 1
        for _ in range(max(1, n // 4)):
            out.append((R, rng.integers(0, cur)))
            cur -= 1
            out.append((U, rng.integers(0, cur)))
        return out
    raise AssertionError(kind)


def _shape(S, n):
    if n in (3, 4, 5, 12):
        counts = {3: [130, 0, 65], 4: [64, 1, 63, 0], 5: [65, 130, 0, 1, 64], 12: LENS + LENS[::-1]}[n]
        return _lens_scene(700 + n + S, counts, S)
    return _scene(8100 + 3 * n + S, n, (3, 20) if n == 1 else (0, 9) if n < 100 else (0, 5), S)


@pytest.mark.parametrize("S,n", [(0, 1), (2, 3), (0, 4), (2, 5), (0, 12), (2, 12), (0, 64), (2, 65), (0, 257), (2, 1025)])
def test_table_equals_the_model(S, n):
    sc, bits = _shape(S, n)
    rng = np.random.default_rng(n * 7 + S)
    t = ba.Table(sc["bound"], S, n, bits)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    with _ctx(sc, sc["nodes"], sc["fit"], sc["bound"], bits) as ctx:
        total = 0
        for step, kind in enumerate(("grow", "equal", "cancel", "many", "shrink", "equal")):
            where = f"S={S} n={n} step {step} ({kind}, {nl.n} nodes)"
            cap = (None, 0, 1, None, 3, None)[step]
            dropped = _surgery(ctx, nl, t, _steps(rng, nl.n, kind), cap, where)
            total += dropped.size
        # a prefix shorter than the truth: remove the node with the longest list, ask for all but one of its ids
        per = np.bincount(t.node, minlength=t.n)
        if per.max(initial=0) >= 2:
            k = int(np.argmax(per))
            dropped = _surgery(ctx, nl, t, [(A, 0), (R, k)], int(per[k]) - 1, f"S={S} n={n} short prefix")
            assert dropped.size == per[k]
            total += dropped.size
        assert total > 0 or n == 1, "no entry ever left: the scene showed nothing"


@pytest.mark.parametrize("S,n", [(2, 5), (0, 65), (2, 257), (0, 1025)])
def test_answers_equal_a_context_that_loaded_the_new_list(S, n):
    sc, bits = _shape(S, n)
    rng = np.random.default_rng(n + S)
    t = ba.Table(sc["bound"], S, n, bits)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    victims = 0
    with _ctx(sc, sc["nodes"], sc["fit"], sc["bound"], bits) as ctx:
        _surgery(ctx, nl, t, _steps(rng, nl.n, "many"), None, f"S={S} n={n} many")
        _check_vs_load(sc, nl, ctx, t, f"S={S} n={n} many", commit=False)
        _surgery(ctx, nl, t, _steps(rng, nl.n, "grow") + _steps(rng, nl.n + 2, "equal"), 0, f"S={S} n={n} grow + equal")
        res = _check_vs_load(sc, nl, ctx, t, f"S={S} n={n} grow + equal")
        victims += _evict(t, res)
        _check_table(ctx, t, f"S={S} n={n} after the commit")
        # the compacted table follows the next surgery too
        _surgery(ctx, nl, t, _steps(rng, nl.n, "shrink"), None, f"S={S} n={n} shrink after the commit")
        _check_vs_load(sc, nl, ctx, t, f"S={S} n={n} shrink after the commit", commit=False)
    assert n < 64 or victims > 0, "no preemptor found a victim: the comparison with the load showed nothing"


def test_the_equal_count_case():
    """REMOVE 0 + APPEND: the stale-table test sees the same count; the followed table answers as the loaded one, and the model says
    that the table left as it was would have answered differently"""
    S, n = 0, 65
    sc, bits = _shape(S, n)
    t = ba.Table(sc["bound"], S, n, bits)
    stale = ba.Table(sc["bound"], S, n, bits)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    with _ctx(sc, sc["nodes"], sc["fit"], sc["bound"], bits) as ctx:
        _surgery(ctx, nl, t, [(R, 0), (A, 7)], None, "equal count")
        assert ctx.n == n and t.n == n
        got = _check_vs_load(sc, nl, ctx, t, "equal count", commit=False)
        req, pres = ctx.read_node_requests()
    nodes = nl.nodes(req, pres)
    answers = []
    for tab in (t, stale):
        eq, keep, ebits = tab.equivalent()
        exp = pp.preempt_pdb_np(pp.PdbPrep(nodes, eq, S, ebits), nl.fit(), sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], CAP)
        answers.append(_map(exp, keep))
    _compare(got, answers[0], "equal count: the device against the reference on the shifted table")
    assert any(not np.array_equal(answers[0][f], answers[1][f]) for f in ("node", "victims", "n_victims")), \
        "the unshifted table answers the same: the scene cannot tell the difference"


def test_a_chain_of_twenty_rounds():
    S, n = 2, 10
    sc, bits = _scene(4321, n, (10, 40), S, q=60, groups=0)
    pool = _ungrouped_pool(1234, n, 20, S)
    rng = np.random.default_rng(21)
    t = ba.Table(sc["bound"], S, n, bits)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    kinds = ["apply", "nodes", "commit", "pdb", "nodes"] * 4
    evicted, dead = 0, []
    with _ctx(sc, sc["nodes"], sc["fit"], sc["bound"], bits) as ctx:
        for step, kind in enumerate(kinds):
            where = f"round {step} ({kind})"
            if kind == "apply":
                rem = rng.permutation(t.id)[: int(rng.integers(0, 12))]
                ni = int(rng.integers(1, 25))
                ins = _take(pool, rng.integers(0, pool.b, ni), rng.integers(0, t.n, ni))
                pdb = rng.integers(0, 2, ni)
                assert ctx.bound_apply(rem, ins, pdb) == t.apply(rem, ins, pdb), where
            elif kind == "nodes":
                what = ("equal", "many", "cancel", "grow", "shrink")[int(rng.integers(0, 5))]
                dead += _surgery(ctx, nl, t, _steps(rng, nl.n, what), None, f"{where} {what}").tolist()
            elif kind == "pdb":
                b2 = rng.integers(0, 2, t.ids).astype(np.uint8) if step % 2 else None
                ctx.bound_pdb_set(b2)
                t.set_pdb(b2)
            else:
                res = _check_vs_load(sc, nl, ctx, t, where, sel=slice(3 * step - 6, 3 * step + 6))
                evicted += _evict(t, res)
            _check_table(ctx, t, where)
        assert dead and evicted > 0 and t.ids > sc["bound"].b and t.count > 0
        # a dropped id is dead: removing it is refused and changes nothing
        before = _state(ctx)
        with pytest.raises(bsa.BsError) as e:
            ctx.bound_apply([dead[0]], None)
        assert e.value.status == -1
        _same_state(before, _state(ctx), "a dropped id removed through bound_apply")
        _check_table(ctx, t, "after the refused remove")


def test_errors_leave_everything_unchanged():
    S, n = 2, 20
    sc, bits = _scene(6, n, (3, 12), S)
    t = ba.Table(sc["bound"], S, n, bits)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(sc["nodes"], sc["fit"])
        with pytest.raises(bsa.BsError) as e:
            ctx.bound_nodes_apply([U], [0])                                     # before load_bound
        assert e.value.status == -4
    with _ctx(sc, sc["nodes"], sc["fit"], sc["bound"], bits) as ctx:
        ask = lambda: ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=CAP)      # noqa: E731
        before, answer = _state(ctx), ask()

        def unchanged(name):
            _same_state(before, _state(ctx), name)
            _compare(ask(), answer, name)
        nd, ids = ctx.bound_nodes_apply([], [], 4)                              # count == 0 with equal counts: fine, nothing changes
        assert nd == 0 and ids.size == 0
        unchanged("an empty list")
        refused = {"a kind outside the three": ([U, 3], [0, 0]), "an update index at the count": ([U], [n]),
                   "a remove index at the count": ([R], [n]), "a remove index at the count of its point": ([R, R], [0, n - 1]),
                   "an update of a node removed in front of it": ([A, R, R, U], [0, n, 0, n - 1]), "every node and one more": ([R] * (n + 1), [0] * (n + 1))}
        for name, (kinds, idx) in refused.items():
            with pytest.raises(bsa.BsError) as e:
                ctx.bound_nodes_apply(kinds, idx, 8)
            assert e.value.status == -1, name
            unchanged(name)
        one, out, nd = (ctypes.c_uint32 * 1)(U), (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
        assert ctx._lib.bs_bound_nodes_apply(ctx._h, 1, None, one, 0, None, ctypes.byref(nd)) == -1            # NULL kind
        assert ctx._lib.bs_bound_nodes_apply(ctx._h, 1, one, None, 0, None, ctypes.byref(nd)) == -1            # NULL index
        assert ctx._lib.bs_bound_nodes_apply(ctx._h, 1, one, one, 4, None, ctypes.byref(nd)) == -1             # NULL dropped_ids with a cap
        assert ctx._lib.bs_bound_nodes_apply(ctx._h, 1, one, one, 4, out, None) == 0                           # NULL n_dropped_out is fine (UPDATE 0)
        unchanged("NULL arrays")
        # lists that are not what the node list got: the replay ends at another count
        for name, (kinds, idx) in {"a remove nobody made": ([R], [0]), "an append nobody made": ([A], [0])}.items():
            with pytest.raises(bsa.BsError) as e:
                ctx.bound_nodes_apply(kinds, idx)
            assert e.value.status == -4, name
            unchanged(name)
        ctx.set_shard(0, 2)
        with pytest.raises(bsa.BsError) as e:
            ctx.bound_nodes_apply([U], [0])
        assert e.value.status == -4
        ctx.set_shard(0, 1)
        unchanged("a sharded context")
        # surgery without the new call: the preemption calls and bs_bound_apply refuse the table, an empty or a wrong list does not mend it
        ctx.apply_node_deltas([nl.remove(3)])
        for call in (ask, lambda: ctx.bound_apply([int(t.id[0])], None), lambda: ctx.bound_nodes_apply([], []), lambda: ctx.bound_nodes_apply([A], [0]),
                     lambda: ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=CAP, apply=True)):
            with pytest.raises(bsa.BsError) as e:
                call()
            assert e.value.status == -4
        _same_state(before, _state(ctx), "refused after the surgery")
        nd, ids = ctx.bound_nodes_apply([R], [3], 1)
        _, dropped, _ = bn.nodes_apply(t, [R], [3], n_expected=n - 1)
        assert nd == dropped.size and np.array_equal(ids, dropped[:1])
        _check_table(ctx, t, "after the refused calls")
        _check_vs_load(sc, nl, ctx, t, "after the refused calls")


def test_from_an_empty_table_and_down_to_one():
    S = 2
    # appends only, from an empty table: the new nodes take inserts
    sc, _ = _scene(78, 3, 4, S)
    pool = sc["bound"]
    empty = soa.Bound.empty(0, 4 + S)
    t = ba.Table(empty, S, 3)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    with _ctx(sc, sc["nodes"], sc["fit"], empty) as ctx:
        dropped = _surgery(ctx, nl, t, [(A, 0), (A, 1)], 4, "appends on an empty table")
        assert dropped.size == 0 and ctx.bound_count() == 0 and ctx.bound_ids() == 0 and t.n == 5
        ins = _take(pool, np.arange(pool.b), np.arange(pool.b) % 5)
        assert ctx.bound_apply([], ins) == t.apply([], ins) == 0
        _check_table(ctx, t, "inserts on appended nodes")
        _check_vs_load(sc, nl, ctx, t, "inserts on appended nodes", commit=False)
    # every node that holds pods leaves, nodes without pods stay
    counts = [0, 5, 0, 70, 0]
    sc, bits = _lens_scene(79, counts, S)
    t = ba.Table(sc["bound"], S, 5, bits)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    with _ctx(sc, sc["nodes"], sc["fit"], sc["bound"], bits) as ctx:
        dropped = _surgery(ctx, nl, t, [(R, 3), (U, 3), (R, 1)], None, "down to an empty table")
        assert dropped.size == 75 and ctx.bound_count() == 0 and ctx.bound_ids() == 75 and ctx.n == 3
        res = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=4)
        assert not res["n_victims"].any()
        pool = _ungrouped_pool(80, 3, 3, S)
        ins = _take(pool, np.arange(pool.b))
        assert ctx.bound_apply([], ins) == t.apply([], ins) == 75
        _check_table(ctx, t, "refilled")
        _check_vs_load(sc, nl, ctx, t, "refilled", commit=False)


def test_hand_known_answers_on_the_device():
    for sc in bn.hand_kats():
        n = sc["n"]
        nodes = soa.Nodes(np.full((4, n), 1 << 40, np.int64), np.zeros((4, n), np.int64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8))
        fit = soa.FitMasks.from_bool(np.ones((1, n), bool))
        nl = bn.NodeList(nodes, fit)
        with bsa.Context(scalar_lanes=0, device=0) as ctx:
            ctx.load_nodes(nodes, fit)
            ctx.load_bound(ba.kat_bound(sc["bound"]))
            for i, st in enumerate(sc["steps"]):
                where = (sc["name"], i)
                if "kind" in st:
                    deltas = [nl.append(0) if k == A else nl.remove(j) if k == R else nl.update(j) for k, j in zip(st["kind"], st["index"])]
                    ctx.apply_node_deltas(deltas)
                    nd, ids = ctx.bound_nodes_apply(st["kind"], st["index"], 8)
                    assert ctx.n == st["n"] and nd == len(st["dropped"]) and ids.tolist() == st["dropped"], (where, nd, ids.tolist())
                elif "error" in st:
                    with pytest.raises(bsa.BsError) as e:
                        ctx.bound_apply(st["remove"], ba.kat_bound(st["insert"]))
                    assert e.value.status == st["error"], where
                else:
                    assert ctx.bound_apply(st["remove"], ba.kat_bound(st["insert"])) == st["first_id"], where
                ids, nd = ctx.read_bound()
                assert ids.tolist() == st["id"] and nd.tolist() == st["node"], (where, ids.tolist(), nd.tolist())
