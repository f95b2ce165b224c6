"""GPU tests of bs_bound_apply / bs_bound_ids / bs_bound_dump: the resident bound table patched on the device equals the numpy model of
tests/bound_apply_ref.py (every column, the PDB bits included) and equals a second context that LOADED the equivalent table — the
surviving and the new entries in ascending id order — in what bs_preempt_run and bs_preempt_commit(APPLY) answer on it, victims mapped
through the monotone id map.  Shapes are the smallest at which each piece can go wrong: node counts around the scan's thread split
(1024 threads) and the merge's four nodes per workgroup, per-node lengths around the 64-entry windows before and after the delta."""
import importlib

import numpy as np
import pytest

import bound_apply_ref as ba
import preempt_pdb_ref as pp
from preempt_scenes import groups_for

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth = bsa.soa, bsa.synth
FIELDS = pp.FIELDS
CAP = 300


def _scene(seed, n, per, S, q=24, groups=6):
    sc, bits = pp.pdb_scene(seed, n, per, S, q, groups, 0.4)
    return sc, bits


def _trim(sc, counts):
    """the scene's bound table cut to counts[k] entries on node k (its first ones)"""
    b = sc["bound"]
    keep = np.concatenate([np.nonzero(b.node == k)[0][:c] for k, c in enumerate(counts)]).astype(np.int64)
    sc["bound"] = soa.Bound(b.node[keep], b.priority[keep], b.start_ns[keep], b.group[keep], b.req[:, keep], b.req_present[keep])
    return sc


def _ctx(sc, bound=None, bits=None, nodes=None):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"] if nodes is None else nodes, sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"] if bound is None else bound)
    if bits is not None:
        ctx.bound_pdb_set(bits)
    return ctx


def _state(ctx):
    ids, nodes = ctx.read_bound()
    return dict(ctx.bound_dump(), id=ids, node=nodes, ids=np.array([ctx.bound_ids()]), count=np.array([ctx.bound_count()]))


def _same_state(a, b, where):
    for f in a:
        assert np.array_equal(a[f], b[f]), f"{where}: {f} changed"


def _check_table(ctx, t, where):
    """read_bound and bound_dump against the model, every column"""
    tab = t.table()
    ids, nodes = ctx.read_bound()
    assert ctx.bound_count() == t.count and ctx.bound_ids() == t.ids, f"{where}: count {ctx.bound_count()} / ids {ctx.bound_ids()} vs {t.count} / {t.ids}"
    assert np.array_equal(ids, tab["id"]), f"{where}: ids {ids[:40]} vs {tab['id'][:40]}"
    assert np.array_equal(nodes, tab["node"]), f"{where}: nodes"
    dump = ctx.bound_dump()
    for f in ba.COLUMNS:
        assert np.array_equal(dump[f], tab[f]), f"{where}: column {f}"


def _map(res, keep):
    out = dict(res)
    out["victims"] = np.where(np.arange(res["victims"].shape[1])[None] < np.minimum(res["n_victims"], res["victims"].shape[1])[:, None],
                              keep[res["victims"]] if keep.size else 0, 0).astype(np.uint32)
    return out


def _compare(got, exp, where):
    for f in FIELDS:
        if not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(np.any((got[f] != exp[f]).reshape(len(got[f]), -1), axis=1))[0]
            i = int(bad[0])
            pytest.fail(f"{where}: {f} differs at preemptor {i} of {len(bad)} bad: got {got[f][i]} expected {exp[f][i]}")


def _check_vs_reload(sc, ctx, t, where, commit=True, assume=False, sel=slice(None)):
    """a second context loads the equivalent table (and the patched context's node requests): same table through the id map, same
    answers of preempt() and, with commit, of preempt_commit(apply=True) and the same state after it.  Returns the patched context's
    commit result."""
    eq, keep, bits = t.equivalent()
    req, pres = ctx.read_node_requests()
    nodes = soa.Nodes(sc["nodes"].allocatable, req, sc["nodes"].allocatable_present, pres, sc["nodes"].flags)
    pi, pr = sc["pod_index"][sel], sc["priority"][sel]
    with _ctx(sc, eq, bits, nodes) as ref:
        ids_a, nodes_a = ctx.read_bound()
        ids_b, nodes_b = ref.read_bound()
        assert np.array_equal(keep[ids_b] if keep.size else ids_b, ids_a) and np.array_equal(nodes_a, nodes_b), f"{where}: table vs the reload"
        da, db = ctx.bound_dump(), ref.bound_dump()
        for f in ba.COLUMNS:
            assert np.array_equal(da[f], db[f]), f"{where}: column {f} vs the reload"
        got = ctx.preempt(pi, pr, sc["protected"], victim_cap=CAP)
        _compare(got, _map(ref.preempt(pi, pr, sc["protected"], victim_cap=CAP), keep), f"{where}: preempt vs the reload")
        if not commit:
            return got
        got = ctx.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP, apply=True, assume=assume)
        assert got["n_victims"].max(initial=0) <= CAP
        _compare(got, _map(ref.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP, apply=True, assume=assume), keep), f"{where}: commit vs the reload")
        ra, rb = ctx.read_node_requests(), ref.read_node_requests()
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), f"{where}: node requests after the commit"
        ids_a, nodes_a = ctx.read_bound()
        ids_b, nodes_b = ref.read_bound()
        assert np.array_equal(keep[ids_b] if keep.size else ids_b, ids_a) and np.array_equal(nodes_a, nodes_b), f"{where}: table after the commit"
        da, db = ctx.bound_dump(), ref.bound_dump()
        for f in ba.COLUMNS:
            assert np.array_equal(da[f], db[f]), f"{where}: column {f} after the commit"
    return got


def _ungrouped_pool(seed, n, per, S):
    """entries to insert into a scene without groups (with tens of pods per node, one protected or missing-group pod among the potential
    victims refuses the node, and no preemptor would find a victim)"""
    pool, _ = synth.make_bound(seed, n, 1, per, S, levels=pp.PDB_LEVELS)
    pool.group[:] = soa.POD_NOT_GROUPED
    return pool


def _evict(t, res):
    v = [res["victims"][i, : int(res["n_victims"][i])] for i in range(len(res["node"])) if res["node"][i] >= 0]
    t.evict(np.concatenate(v) if v else [])
    return int(sum(len(x) for x in v))


def _take(pool, idx, node=None):
    idx = np.asarray(idx, np.int64)
    return soa.Bound(pool.node[idx] if node is None else np.asarray(node, np.uint32), pool.priority[idx], pool.start_ns[idx], pool.group[idx],
                     pool.req[:, idx], pool.req_present[idx])


def _delta(kind, rng, t, pool, n):
    """(remove ids, insert Bound or None) of one kind, against the model's live entries"""
    live = t.id.copy()
    draw = lambda c: rng.integers(0, pool.b, c)                                # noqa: E731
    if kind == "none":
        return [], None
    if kind == "ins":
        return [], _take(pool, draw(n // 3 + 5), rng.integers(0, n, n // 3 + 5))
    if kind == "rem":
        return rng.permutation(live)[: max(1, live.size // 5)] if live.size else [], None
    if kind == "one":                                                           # both on the same node
        k = int(t.node[rng.integers(0, t.count)]) if t.count else 0
        on = live[t.node == k]
        return rng.permutation(on)[: (on.size + 1) // 2], _take(pool, draw(5), np.full(5, k))
    if kind == "every":                                                         # every node: one in, and one out where it holds any
        first = [int(live[t.node == k][0]) for k in range(n) if np.any(t.node == k)] if n <= 100 else \
            live[np.unique(t.node, return_index=True)[1]].tolist()
        return rng.permutation(first), _take(pool, draw(n), rng.permutation(n))
    if kind == "wipe_node":
        k = int(t.node[rng.integers(0, t.count)]) if t.count else 0
        return live[t.node == k], None
    if kind == "wipe_all":
        return rng.permutation(live), None
    raise AssertionError(kind)


SHAPES = [(0, 1, (3, 20)), (1, 3, (0, 70)), (4, 64, (0, 9)), (12, 65, (0, 9)), (0, 1023, (0, 5)), (1, 1025, (0, 5)), (4, 3000, (0, 4)), (12, 3000, (0, 3))]


@pytest.mark.parametrize("S,n,per", SHAPES)
def test_apply_equals_the_model_and_the_reload(S, n, per):
    sc, bits = _scene(8000 + 3 * n + S, n, per, S)
    pool, _ = synth.make_bound(31 + n + S, n, sc["groups"], 3, S)
    rng = np.random.default_rng(n * 13 + S)
    t = ba.Table(sc["bound"], S, n, bits)
    victims = 0
    with _ctx(sc, bits=bits) as ctx:
        for step, kind in enumerate(("none", "ins", "rem", "one", "every", "wipe_node", "ins")):
            rem, ins = _delta(kind, rng, t, pool, n)
            pdb = None if ins is None or step % 2 else rng.integers(0, 2, ins.b)
            where = f"S={S} n={n} step {step} ({kind})"
            first = ctx.bound_apply(rem, ins, pdb)
            assert first == t.apply(rem, ins, pdb), where
            _check_table(ctx, t, where)
            if kind in ("one", "every"):
                _check_vs_reload(sc, ctx, t, where, commit=False)
        res = _check_vs_reload(sc, ctx, t, f"S={S} n={n} end")
        victims += _evict(t, res)
        _check_table(ctx, t, f"S={S} n={n} after the commit")
        # a removed and an evicted id are gone for good; the table goes down to empty and comes back
        rem, _ = _delta("wipe_all", rng, t, pool, n)
        ctx.bound_apply(rem, None)
        t.apply(rem, None)
        assert ctx.bound_count() == 0
        _check_table(ctx, t, "emptied")
        rem, ins = _delta("ins", rng, t, pool, n)
        assert ctx.bound_apply(rem, ins) == t.apply(rem, ins)
        _check_table(ctx, t, "refilled")
        _check_vs_reload(sc, ctx, t, f"S={S} n={n} refilled", commit=False)
    assert n < 64 or victims > 0, "no preemptor found a victim: the comparison with the reload showed nothing"


@pytest.mark.parametrize("S", [1, 12])
def test_lengths_around_the_windows_before_and_after(S):
    counts = [0, 1, 63, 64, 65, 129] * 2
    n = len(counts)
    sc, bits = _scene(515 + S, n, 130, S, groups=0)
    sc = _trim(sc, counts)
    bits = bits[: sc["bound"].b]
    pool = _ungrouped_pool(99 + S, n, 80, S)
    rng = np.random.default_rng(S)
    t = ba.Table(sc["bound"], S, n, bits)
    with _ctx(sc, bits=bits) as ctx:
        # one more on the first six nodes (0->1, 1->2, 63->64, 64->65, 65->66, 129->130), one less on the others (1->0, ..., 65->64, 129->128)
        rem = [int(rng.choice(t.id[t.node == k])) for k in range(6, 12) if counts[k]]
        ins = _take(pool, rng.integers(0, pool.b, 6), np.arange(6))
        assert ctx.bound_apply(rem, ins, np.ones(6)) == t.apply(rem, ins, np.ones(6))
        _check_table(ctx, t, "plus / minus one")
        assert np.bincount(t.node, minlength=n).tolist() == [1, 2, 64, 65, 66, 130, 0, 0, 62, 63, 64, 128]
        _check_vs_reload(sc, ctx, t, "plus / minus one", commit=False)
        # more inserts than one window on a node of more than one window, three of its entries leaving; node 10 back to 65 and 63 -> 64
        rem = rng.permutation(t.id[t.node == 5])[:3]
        nodes = np.concatenate([np.full(70, 5), [10], [9]])
        ins = _take(pool, rng.integers(0, pool.b, nodes.size), nodes)
        pdb = rng.integers(0, 2, nodes.size)
        assert ctx.bound_apply(rem, ins, pdb) == t.apply(rem, ins, pdb)
        _check_table(ctx, t, "seventy on one node")
        # a whole node's list leaves (130 + 70 - 3 entries), another is filled from empty past two windows
        rem = t.id[t.node == 5]
        ins = _take(pool, rng.integers(0, pool.b, 129), np.full(129, 6))
        assert ctx.bound_apply(rem, ins) == t.apply(rem, ins)
        _check_table(ctx, t, "a node emptied, a node filled")
        res = _check_vs_reload(sc, ctx, t, "lengths end")
        assert _evict(t, res) > 0 or S == 12          # (at 12 scalar lanes few nodes hold every key a preemptor asks for)
        _check_table(ctx, t, "lengths after the commit")


def test_from_an_empty_table():
    S, n = 1, 9
    sc, _ = _scene(77, n, 4, S)
    pool = sc["bound"]
    rng = np.random.default_rng(7)
    empty = soa.Bound.empty(0, 4 + S)
    t = ba.Table(empty, S, n)
    with _ctx(sc, empty) as ctx:
        assert ctx.bound_ids() == 0 and ctx.bound_apply([], None) == 0
        ins = _take(pool, rng.permutation(pool.b))                              # the scene's own pods arrive one event batch at a time
        half = ins.b // 2
        for part in (np.arange(half), np.arange(half, ins.b)):
            p = _take(ins, part)
            assert ctx.bound_apply([], p) == t.apply([], p)
            _check_table(ctx, t, "from empty")
        res = _check_vs_reload(sc, ctx, t, "from empty")
        assert _evict(t, res) > 0
        ctx.bound_apply(t.id, None)
        t.apply(t.id, None)
        _check_table(ctx, t, "down to empty")
        assert ctx.bound_count() == 0 and ctx.bound_ids() == pool.b
        res = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=4)
        assert not res["n_victims"].any()


def test_tie_rules_on_the_device():
    for sc in ba.hand_kats():
        n = sc["n"]
        nodes = soa.Nodes(np.full((4, n), 1 << 40, np.int64), np.zeros((4, n), np.int64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8))
        with bsa.Context(scalar_lanes=0, device=0) as ctx:
            ctx.load_nodes(nodes, soa.FitMasks.from_bool(np.ones((1, n), bool)))
            ctx.load_bound(ba.kat_bound(sc["bound"]))
            for i, st in enumerate(sc["steps"]):
                first = ctx.bound_apply(st["remove"], ba.kat_bound(st["insert"]))
                ids, nd = ctx.read_bound()
                assert first == st["first_id"] and ids.tolist() == st["id"] and nd.tolist() == st["node"], (sc["name"], i, ids.tolist(), nd.tolist())


def test_capacity_exactly_the_limit_then_one_more():
    S, n = 1, 2
    sc, bits = _scene(21, n, 5, S, q=4)
    pool, _ = synth.make_bound(22, n, sc["groups"], 40, S)
    t = ba.Table(sc["bound"], S, n, bits)
    with _ctx(sc, bits=bits) as ctx:
        fill = ba.MAX_PER_NODE - int((t.node == 0).sum())
        ins = _take(pool, np.arange(fill) % pool.b, np.zeros(fill))
        assert ctx.bound_apply([], ins) == t.apply([], ins)
        _check_table(ctx, t, "exactly BS_BOUND_MAX_PER_NODE")
        before = _state(ctx)
        one = _take(pool, [0], [0])
        with pytest.raises(bsa.BsError) as e:
            ctx.bound_apply([], one)
        assert e.value.status == -5
        _same_state(before, _state(ctx), "one over the limit")
        gone = t.id[t.node == 0][:1]                                            # one out, one in on the full node: still exactly the limit
        assert ctx.bound_apply(gone, one) == t.apply(gone, one)
        _check_table(ctx, t, "full node, one out and one in")


def test_errors_leave_everything_unchanged():
    S, n = 1, 20
    sc, bits = _scene(5, n, (3, 12), S)
    pool, _ = synth.make_bound(6, n, sc["groups"], 3, S)
    t = ba.Table(sc["bound"], S, n, bits)
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(sc["nodes"], sc["fit"])
        with pytest.raises(bsa.BsError) as e:
            ctx.bound_apply([], _take(pool, [0]))                               # before load_bound
        assert e.value.status == -4
    with _ctx(sc, bits=bits) as ctx:
        res = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=CAP, apply=True)
        evicted = np.concatenate([res["victims"][i, : int(res["n_victims"][i])] for i in range(len(res["node"]))])
        assert evicted.size
        t.evict(evicted)
        removed = t.id[::7][:3].copy()
        ins = _take(pool, [1, 2, 3])
        assert ctx.bound_apply(removed, ins) == t.apply(removed, ins)
        _check_table(ctx, t, "before the refused calls")
        before = _state(ctx)
        live = t.id[:4]
        bad_node, bad_group = _take(pool, [0], [n]), _take(pool, [0])
        bad_group.group[0] = soa.POD_GROUP_MISSING - 1
        refused = {"an unknown id": ([t.ids], None), "an unknown id among live ones": (list(live) + [t.ids + 5], ins),
                   "an evicted id": ([int(evicted[0])], None), "an id removed earlier": ([int(removed[1])], ins),
                   "a duplicate id": ([int(live[0]), int(live[1]), int(live[0])], None), "a node >= n": ([int(live[0])], bad_node),
                   "a bad group": ([], bad_group)}
        for name, (rem, new) in refused.items():
            with pytest.raises(bsa.BsError) as e:
                ctx.bound_apply(rem, new)
            assert e.value.status == -1, name
            _same_state(before, _state(ctx), name)
        assert ctx._lib.bs_bound_apply(ctx._h, None, None) == -1
        d = soa.BoundDeltaStruct(1, None, 0, None, None, None, None, None, None, None)
        assert ctx._lib.bs_bound_apply(ctx._h, __import__("ctypes").byref(d), None) == -1      # NULL required array
        _same_state(before, _state(ctx), "NULL arrays")
        assert ctx.bound_apply(live, ins) == t.apply(live, ins)                 # and the context still works
        _check_table(ctx, t, "after the refused calls")
        _check_vs_reload(sc, ctx, t, "after the refused calls", commit=False)


def test_pdb_bits_follow_the_delta():
    S, n = 1, 30
    sc, bits = _scene(2024, n, (4, 14), S, q=40)
    pool, _ = synth.make_bound(9, n, sc["groups"], 3, S, levels=pp.PDB_LEVELS)
    rng = np.random.default_rng(3)
    t = ba.Table(sc["bound"], S, n, bits)
    with _ctx(sc, bits=bits) as ctx:
        # two low-priority newcomers per node, half of them violating
        ins = _take(pool, rng.integers(0, pool.b, 2 * n), np.repeat(np.arange(n), 2))
        ins.priority[:] = np.minimum(ins.priority, 100)
        pdb = np.tile([1, 0], n)
        rem = rng.permutation(t.id)[: t.count // 6]
        first = ctx.bound_apply(rem, ins, pdb)
        assert first == t.apply(rem, ins, pdb)
        _check_table(ctx, t, "pdb delta")
        eq, keep, ebits = t.equivalent()
        got = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=32)
        exp = pp.preempt_pdb_np(pp.PdbPrep(sc["nodes"], eq, S, ebits), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], 32)
        _compare(got, _map(exp, keep), "preempt against the reference on the equivalent table")
        assert got["n_pdb_violations"].any()
        lists = [got["victims"][i, : min(int(got["n_victims"][i]), 32)] for i in range(len(got["node"]))]
        vbit = {int(i): int(b) for i, b in zip(t.id, t.pdb)}
        assert any(int(i) >= first and vbit[int(i)] for v in lists for i in v), "no inserted violating entry among the victims"
        # the grown id space: bits for every id, the old size is refused
        with pytest.raises(bsa.BsError) as e:
            ctx.bound_pdb_set(np.zeros(sc["bound"].b, np.uint8))
        assert e.value.status == -1
        bits2 = rng.integers(0, 2, t.ids).astype(np.uint8)
        ctx.bound_pdb_set(bits2)
        t.set_pdb(bits2)
        _check_table(ctx, t, "bound_pdb_set over the grown id space")
        # a node loses all its violating pods: no bit left there, one reprieve pass again, answers as the reload's
        k = int(np.argmax(np.bincount(t.node[t.pdb != 0], minlength=n)))
        rem = t.id[(t.node == k) & (t.pdb != 0)]
        assert rem.size and np.any((t.node == k) & (t.pdb == 0))
        ctx.bound_apply(rem, None)
        t.apply(rem, None)
        _check_table(ctx, t, "violating pods of one node removed")
        ids, nodes = ctx.read_bound()
        assert not ctx.bound_dump()["pdb"][nodes == k].any()
        res = _check_vs_reload(sc, ctx, t, "violating pods of one node removed")
        assert res["n_pdb_violations"].any()


def test_a_chain_of_twenty_steps():
    S, n = 1, 10
    sc, bits = _scene(1234, n, (10, 40), S, q=60, groups=0)
    pool = _ungrouped_pool(4321, n, 20, S)
    rng = np.random.default_rng(20)
    t = ba.Table(sc["bound"], S, n, bits)
    kinds = ["apply", "commit", "apply", "pdb", "assume"] * 4
    evicted = 0
    with _ctx(sc, bits=bits) as ctx:
        for step, kind in enumerate(kinds):
            where = f"step {step} ({kind})"
            if kind == "apply":
                rem = rng.permutation(t.id)[: int(rng.integers(0, 12))]
                ni = int(rng.integers(0, 25))
                ins = _take(pool, rng.integers(0, pool.b, ni), rng.integers(0, n, ni)) if ni else None
                pdb = rng.integers(0, 2, ni) if ni else None
                assert ctx.bound_apply(rem, ins, pdb) == t.apply(rem, ins, pdb), where
            elif kind == "pdb":
                b2 = rng.integers(0, 2, t.ids).astype(np.uint8) if step % 2 else None
                ctx.bound_pdb_set(b2)
                t.set_pdb(b2)
            else:
                sel = slice(3 * step, 3 * step + 3)
                res = _check_vs_reload(sc, ctx, t, where, assume=kind == "assume", sel=sel)
                evicted += _evict(t, res)
            _check_table(ctx, t, where)
    assert evicted > 0 and t.ids > sc["bound"].b


def test_flat_form_equals_the_struct_form():
    S, n = 4, 17
    sc, bits = _scene(88, n, (0, 9), S)
    pool, _ = synth.make_bound(89, n, sc["groups"], 3, S)
    rng = np.random.default_rng(8)
    rem = rng.permutation(sc["bound"].b)[:9]
    ins = _take(pool, rng.integers(0, pool.b, 11), rng.integers(0, n, 11))
    pdb = rng.integers(0, 2, 11)
    states = []
    for flat in (False, True):
        with _ctx(sc, bits=bits) as ctx:
            assert ctx.bound_apply(rem, ins, pdb, flat=flat) == sc["bound"].b
            states.append(_state(ctx))
    _same_state(states[0], states[1], "flat vs struct")
    t = ba.Table(sc["bound"], S, n, bits)
    t.apply(rem, ins, pdb)
    assert np.array_equal(states[1]["id"], t.table()["id"])
