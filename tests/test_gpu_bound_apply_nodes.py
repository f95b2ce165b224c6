"""GPU tests of bs_bound_apply_ex: with BS_BOUND_NODES the node requests follow a bound-table delta on the device.  After every step of
a random delta sequence bs_nodes_read and the table equal the models of tests/bound_apply_nodes_ref.py / bound_apply_ref.py bit for bit;
the call equals the sequence it replaces (bs_bound_apply + bs_nodes_assume with vectors computed on the host) in everything later calls
read, the host mirror included; removing a plan's victims equals BS_PREEMPT_APPLY; flags 0 is bs_bound_apply; every refused call leaves
table, ids, PDB bits and node requests as they were.  Shapes: node counts around the four nodes per workgroup and the 256-thread blocks
of k_nodes_assume, old list lengths around the 64-entry windows, 0 / 2 / 12 scalar lanes."""
import importlib

import numpy as np
import pytest

import bound_apply_nodes_ref as bn
import bound_apply_ref as ba
import preempt_pdb_ref as pp
from preempt_scenes import groups_for

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth, capi = bsa.soa, bsa.synth, bsa.capi
FIELDS = pp.FIELDS
NODES = capi.BS_BOUND_NODES
CAP = 300


def _ctx(sc, bits=None):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    if bits is not None:
        ctx.bound_pdb_set(bits)
    return ctx


def _model(sc, bits=None):
    return bn.State(sc["bound"], sc["S"], sc["nodes"].n, sc["nodes"].requested, sc["nodes"].requested_present, bits)


def _state(ctx):
    ids, nodes = ctx.read_bound()
    req, pres = ctx.read_node_requests()
    return dict(ctx.bound_dump(), id=ids, node=nodes, ids=np.array([ctx.bound_ids()]), count=np.array([ctx.bound_count()]), node_req=req, node_pres=pres)


def _same_state(a, b, where):
    for f in a:
        assert np.array_equal(a[f], b[f]), f"{where}: {f} differs"


def _check(ctx, m, where):
    """bs_nodes_read, bs_bound_read and bs_bound_dump against the model, bit for bit"""
    req, pres = ctx.read_node_requests()
    if not np.array_equal(req, m.req):
        l, k = np.argwhere(req != m.req)[0]
        pytest.fail(f"{where}: node requests differ at lane {l} node {k}: got {req[l, k]} expected {m.req[l, k]} ({int((req != m.req).sum())} words)")
    assert np.array_equal(pres, m.pres), f"{where}: present bits differ at nodes {np.nonzero(pres != m.pres)[0][:8]}"
    tab = m.t.table()
    ids, nodes = ctx.read_bound()
    assert ctx.bound_count() == m.t.count and ctx.bound_ids() == m.t.ids, where
    assert np.array_equal(ids, tab["id"]) and np.array_equal(nodes, tab["node"]), f"{where}: table"
    dump = ctx.bound_dump()
    for f in ba.COLUMNS:
        assert np.array_equal(dump[f], tab[f]), f"{where}: column {f}"


def _take(pool, idx, node):
    idx = np.asarray(idx, np.int64)
    return soa.Bound(np.asarray(node, np.uint32), pool.priority[idx], pool.start_ns[idx], pool.group[idx], pool.req[:, idx], pool.req_present[idx])


def _pool(seed, n, S):
    """entries to insert: every scalar key on some of them, large values among the requests (sums that wrap)"""
    pool, _ = synth.make_bound(seed, max(n, 4), 1, 6, S, levels=pp.PDB_LEVELS)
    rng = np.random.default_rng(seed)
    pool.group[:] = soa.POD_NOT_GROUPED
    pool.req_present[:] = rng.integers(0, 1 << S, pool.b)
    big = rng.random(pool.b) < 0.1
    pool.req[0] = np.where(big, rng.integers(1 << 61, (1 << 63) - 1, pool.b, dtype=np.int64), pool.req[0])
    return pool


def _delta(kind, rng, t, pool, n):
    live = t.id
    draw = lambda c: rng.integers(0, pool.b, c)                                # noqa: E731
    if kind == "mixed":
        c = int(rng.integers(1, 9))
        return rng.permutation(live)[: int(rng.integers(0, min(live.size, 8) + 1))], _take(pool, draw(c), rng.integers(0, n, c))
    if kind == "rem":
        return rng.permutation(live)[: max(1, live.size // 5)] if live.size else [], None
    if kind == "ins":
        c = n // 3 + 3
        return [], _take(pool, draw(c), rng.integers(0, n, c))
    if kind == "every":                                                         # every node: one in, and one out where it holds any
        first = live[np.unique(t.node, return_index=True)[1]] if live.size else []
        return rng.permutation(first), _take(pool, draw(n), rng.permutation(n))
    if kind == "one":                                                           # a single node: half its list out, three in
        k = int(t.node[rng.integers(0, t.count)]) if t.count else 0
        on = live[t.node == k]
        return rng.permutation(on)[: (on.size + 1) // 2], _take(pool, draw(3), np.full(3, k))
    if kind == "wipe_node":
        k = int(t.node[rng.integers(0, t.count)]) if t.count else 0
        return live[t.node == k], None
    raise AssertionError(kind)


KINDS = ("mixed", "every", "one", "rem", "ins", "wipe_node", "mixed", "every")


@pytest.mark.parametrize("S,n", [(0, 1), (2, 3), (12, 4), (0, 5), (2, 255), (12, 256), (0, 257)])
def test_node_requests_and_table_equal_the_model_after_every_step(S, n):
    sc, bits = pp.pdb_scene(700 + 3 * n + S, n, (0, 6), S, 8, 0, 0.3)
    sc["nodes"].requested_present[:] = np.random.default_rng(n).integers(0, 1 << S, n)       # keys absent on the node, present on pods
    pool = _pool(40 + n + S, n, S)
    rng = np.random.default_rng(n * 17 + S)
    m = _model(sc, bits)
    assert n <= 600 and sc["bound"].b <= 6000
    with _ctx(sc, bits) as ctx:
        for step, kind in enumerate(KINDS):
            rem, ins = _delta(kind, rng, m.t, pool, n)
            pdb = None if ins is None or step % 2 else rng.integers(0, 2, ins.b)
            where = f"S={S} n={n} step {step} ({kind})"
            assert ctx.bound_apply_ex(rem, ins, pdb, flags=NODES, flat=bool(step % 2)) == m.apply_ex(rem, ins, pdb), where
            _check(ctx, m, where)


@pytest.mark.parametrize("S", [0, 2, 12])
def test_old_list_lengths_around_the_windows(S):
    counts = [0, 1, 63, 64, 65, 129]
    n = len(counts)
    sc, bits = pp.pdb_scene(515 + S, n, 130, S, 8, 0, 0.3)
    b = sc["bound"]
    keep = np.concatenate([np.nonzero(b.node == k)[0][:c] for k, c in enumerate(counts)]).astype(np.int64)
    sc["bound"] = soa.Bound(b.node[keep], b.priority[keep], b.start_ns[keep], b.group[keep], b.req[:, keep], b.req_present[keep])
    bits = bits[keep]
    pool = _pool(99 + S, n, S)
    rng = np.random.default_rng(S)
    m = _model(sc, bits)
    with _ctx(sc, bits) as ctx:
        # every node touched at its old length: the last entry of each list out (the window's last lane), one in
        t = m.t.table()
        rem = [int(t["id"][t["node"] == k][-1]) for k in range(n) if counts[k]]
        ins = _take(pool, rng.integers(0, pool.b, n), np.arange(n))
        assert ctx.bound_apply_ex(rem, ins) == m.apply_ex(rem, ins)
        _check(ctx, m, "one out, one in at every length")
        assert np.bincount(m.t.node, minlength=n).tolist() == [1, 1, 63, 64, 65, 129]
        # removes only: the first entry and every third; then the whole of the longest list, and seventy on the empty-most node
        t = m.t.table()
        rem = np.concatenate([t["id"][t["node"] == k][::3] for k in range(n)])
        assert ctx.bound_apply_ex(rem, None) == m.apply_ex(rem, None)
        _check(ctx, m, "every third out")
        rem = m.t.id[m.t.node == 5]
        ins = _take(pool, rng.integers(0, pool.b, 70), np.zeros(70))
        assert ctx.bound_apply_ex(rem, ins) == m.apply_ex(rem, ins)
        _check(ctx, m, "a list emptied, seventy on one node")


def _host_vectors(req0, pres0, m):
    """what the shim computed itself before: (index, absolute requested lanes, present bits) of every node the delta changed"""
    ch = np.nonzero(np.any(req0 != m.req, axis=0) | (pres0 != m.pres))[0]
    return [(int(k), m.req[:, k].tolist(), int(m.pres[k])) for k in ch]


def _batch(ctx):
    out = ctx.batch(bitmap=True)
    return {f: getattr(out, f) for f in ("pf_code", "pf_first_k", "pf_leader", "fl_code", "fl_feasible", "fl_bitmap", "group_admit", "group_ready")}


@pytest.mark.parametrize("S,n", [(2, 40), (12, 9)])
def test_equals_bound_apply_plus_nodes_assume(S, n):
    sc, bits = pp.pdb_scene(4100 + S, n, (2, 14), S, 16, 0, 0.3)
    pool = _pool(5 + S, n, S)
    rng = np.random.default_rng(S + 1)
    m = _model(sc, bits)
    with _ctx(sc, bits) as a, _ctx(sc, bits) as b:
        for step in range(3):
            live = m.t.id[m.t.node != 0]                                        # node 0 stays untouched
            rem = rng.permutation(live)[: live.size // 6]
            ins = _take(pool, rng.integers(0, pool.b, 12), rng.integers(1, n, 12))
            req0, pres0 = m.req.copy(), m.pres.copy()
            first = m.apply_ex(rem, ins)
            assert a.bound_apply_ex(rem, ins) == first
            assert b.bound_apply(rem, ins) == first
            b.assume_nodes(_host_vectors(req0, pres0, m))
            _check(a, m, f"step {step}")
            _same_state(_state(a), _state(b), f"step {step}")
        ba_, bb_ = _batch(a), _batch(b)
        for f in ba_:
            assert np.array_equal(ba_[f], bb_[f]), f"bs_batch_run: {f}"
        pi, pr = sc["pod_index"], sc["priority"]
        ra, rb = a.preempt(pi, pr, sc["protected"], victim_cap=CAP), b.preempt(pi, pr, sc["protected"], victim_cap=CAP)
        for f in FIELDS:
            assert np.array_equal(ra[f], rb[f]), f"bs_preempt_run: {f}"
        # the host mirror: an UPDATE of the untouched node 0 re-uploads from it
        for ctx in (a, b):
            d = capi.NodeDelta()
            d.kind, d.index = capi.DELTA_UPDATE, 0
            for j in range(4 + S):
                d.allocatable[j], d.requested[j] = int(sc["nodes"].allocatable[j, 0]), int(sc["nodes"].requested[j, 0]) + 1
            d.allocatable_present, d.requested_present, d.flags = int(sc["nodes"].allocatable_present[0]), int(sc["nodes"].requested_present[0]), 0
            d.fit_default, d.n_fit_exceptions = 1, 0
            ctx.apply_node_deltas([d])
        m.req[:, 0] = sc["nodes"].requested[:, 0] + 1
        _check(a, m, "after bs_nodes_apply(UPDATE of an untouched node)")
        _same_state(_state(a), _state(b), "after bs_nodes_apply")
        ra = a.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP, apply=True)
        rb = b.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP, apply=True)
        for f in FIELDS:
            assert np.array_equal(ra[f], rb[f]), f"bs_preempt_commit(APPLY): {f}"
        assert ra["n_victims"].sum() > 0, "no victim: the comparison shows nothing"
        _same_state(_state(a), _state(b), "after the commit")


@pytest.mark.parametrize("S,n", [(0, 30), (4, 30)])
def test_removing_the_victims_equals_preempt_apply(S, n):
    sc, bits = pp.pdb_scene(2024 + S, n, (4, 14), S, 20, 0, 0.3)
    pi, pr = sc["pod_index"], sc["priority"]
    with _ctx(sc, bits) as a, _ctx(sc, bits) as b:
        ra = a.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP, apply=True)
        rb = b.preempt_commit(pi, pr, sc["protected"], victim_cap=CAP)       # the plan only
        for f in FIELDS:
            assert np.array_equal(ra[f], rb[f]), f
        victims = np.concatenate([rb["victims"][i, : int(rb["n_victims"][i])] for i in range(len(pi)) if rb["node"][i] >= 0])
        assert victims.size > 3
        b.bound_apply_ex(victims, None, flags=NODES)
        _same_state(_state(a), _state(b), "BS_PREEMPT_APPLY vs the plan's victims removed with BS_BOUND_NODES")


def test_flags_zero_is_bound_apply():
    S, n = 2, 17
    sc, bits = pp.pdb_scene(88, n, (0, 9), S, 8, 0, 0.3)
    pool = _pool(89, n, S)
    rng = np.random.default_rng(8)
    rem = rng.permutation(sc["bound"].b)[:9]
    ins = _take(pool, rng.integers(0, pool.b, 11), rng.integers(0, n, 11))
    pdb = rng.integers(0, 2, 11)
    states = []
    for call in ("plain", "ex", "ex_flat"):
        with _ctx(sc, bits) as ctx:
            before = ctx.read_node_requests()
            first = ctx.bound_apply(rem, ins, pdb) if call == "plain" else ctx.bound_apply_ex(rem, ins, pdb, flags=0, flat=call == "ex_flat")
            assert first == sc["bound"].b
            after = ctx.read_node_requests()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), f"{call}: node requests moved"
            states.append(_state(ctx))
    _same_state(states[0], states[1], "bs_bound_apply vs bs_bound_apply_ex(0)")
    _same_state(states[0], states[2], "bs_bound_apply vs bs_bound_apply_ex_flat(0)")


def test_errors_leave_everything_unchanged():
    S, n = 2, 20
    sc, bits = pp.pdb_scene(5, n, (3, 12), S, 8, 0, 0.3)
    pool = _pool(6, n, S)
    m = _model(sc, bits)
    with _ctx(sc, bits) as ctx:
        removed = m.t.id[::7][:3].copy()
        ins = _take(pool, [1, 2, 3], [0, 1, 1])
        assert ctx.bound_apply_ex(removed, ins) == m.apply_ex(removed, ins)
        _check(ctx, m, "before the refused calls")
        before = _state(ctx)
        live = m.t.id[:4]
        fill = ba.MAX_PER_NODE + 1 - int((m.t.node == 2).sum())
        over = _take(pool, np.arange(fill) % pool.b, np.full(fill, 2))
        refused = {"a dead id": ([int(removed[1])], ins, NODES, -1), "a dead id among live ones": (list(live) + [int(removed[0])], None, NODES, -1),
                   "an id listed twice": ([int(live[0]), int(live[1]), int(live[0])], ins, NODES, -1),
                   "a node over BS_BOUND_MAX_PER_NODE": ([int(live[0])], over, NODES, -5),
                   "an unknown flag bit": ([int(live[0])], ins, 2, -1), "an unknown flag bit beside the known one": ([int(live[0])], ins, NODES | 4, -1),
                   "the top flag bit": ([], ins, 0x80000000, -1)}
        for name, (rem, new, flags, status) in refused.items():
            for flat in (False, True):
                with pytest.raises(bsa.BsError) as e:
                    ctx.bound_apply_ex(rem, new, flags=flags, flat=flat)
                assert e.value.status == status, name
                _same_state(before, _state(ctx), name)
        assert ctx.bound_apply_ex(live, ins) == m.apply_ex(live, ins)           # and the context still works
        _check(ctx, m, "after the refused calls")
    with bsa.Context(scalar_lanes=S, device=0) as ctx:                          # what bs_bound_apply refuses in this state, with its code
        ctx.load_nodes(sc["nodes"], sc["fit"])
        with pytest.raises(bsa.BsError) as e:
            ctx.bound_apply_ex([], ins)
        assert e.value.status == -4
