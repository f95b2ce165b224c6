"""GPU tests of bs_seq_run_nominated (include/bsched.h, rule S and D6; csrc/bs_seq.hpp, k_seq_pass<TS, true>): the sequential pass with the
resident nominated-pod table in its node choice, against the object-level model tests/seq_nominated_ref.py — every output, the node
requests and group state the pass leaves, the surviving table with its ids, the consumed rows — with the first-fit cursors on and off;
the empty case against bs_seq_run on a twin context; the hand-derived answers; the tile, staging-window and compaction-window edges; what
the calls downstream of the pass see; and every refusal.  Scenes are small (48 to 200 nodes, 80 to 140 pods; the hand scenes a handful);
the models are computed once per scene.  tests/test_seq_nominated_cpu.py asserts that this very scene set is not vacuous — for the cursor
hazards at the granularity of the kernel's cursors (tiles of 64 nodes: the 130- and 200-node scenes and the hand scenes e, f, k, l, m
straddle a tile border), so that the runs with and without cursors walk different search paths."""
import functools
import importlib

import numpy as np
import pytest

import naive_ref as nv
import preempt_pdb_ref as pp
import scenarios
import seq_expire_ref as sx
import seq_nominated_ref as snr
import seq_nominated_scenes as sns
from preempt_scenes import groups_for
from test_gpu_parity import load_ctx
from test_gpu_seq import assert_groups_equal

bsa = importlib.import_module("batch-scheduler_amd")
capi, soa = bsa.capi, bsa.soa
pytestmark = pytest.mark.gpu
NAMES12 = [f"example.com/r{i}" for i in range(12)]
INVALID, STATE = -1, -4


@functools.lru_cache(maxsize=None)
def _case(key):
    """(scene, its SoA, the model's pass): computed once, never changed"""
    kind = key[0]
    if kind == "parity":
        scn = sns.parity_scene(key[1], key[2], key[3])
    elif kind == "kat":
        scn = sns.kat_scene(sns.load_kats()[key[1]], names=scenarios.SCALARS[: key[2]])
    else:
        scn = sns.make(key[1], **dict(key[2]))
    model = snr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], scalar_names=scn["names"])
    return scn, sns.to_soa(scn), model


def _open(parts, rows=True):
    nodes, fit, groups, pods, _, tab = parts
    ctx = load_ctx(bsa, nodes, fit, groups, pods)
    if rows:
        ctx.nominated_load(tab["node"], tab["priority"], tab["req"], tab["req_present"])
    return ctx


def _state(ctx):
    req, pres = ctx.read_node_requests()
    g = ctx.read_groups()
    t = ctx.nominated_read()
    return dict(req=req, pres=pres, matched=g.matched.copy(), flags=g.flags.copy(), sc=g.status_scheduled.copy(), ids=ctx.nominated_ids(),
                **{"t_" + k: v.copy() for k, v in t.items()})


def _same_state(a, b, where):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{where}: {k} changed"


def _check(ctx, key, where, flat=False):
    """one bs_seq_run_nominated on ctx against the model of scene `key`"""
    scn, parts, model = _case(key)
    r = ctx.seq_run_nominated(scn["priority"], scn["own_id"], flat=flat)
    for k in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods"):
        assert r[k].tolist() == list(model[k]), f"{where}: {k}"
    nodes, groups, wait = snr.end_state_soa(model, scn["sc"], soa, dict(parts[4]))
    req, pres = ctx.read_node_requests()
    assert np.array_equal(req, nodes.requested), f"{where}: node requests after the pass (no row in them)"
    assert np.array_equal(pres, nodes.requested_present), f"{where}: node request keys"
    assert_groups_equal(ctx.read_groups(), groups, soa, where)
    assert np.array_equal(ctx.seq_waiting_read(), wait), f"{where}: the pods still waiting at Permit"
    left = snr.objects_to_rows(model["nominees"], scn["names"])
    got = ctx.nominated_read()
    for k in ("id", "node", "priority", "req", "req_present"):
        assert np.array_equal(got[k], left[k]), f"{where}: surviving table, {k}"
    assert ctx.nominated_ids() == len(scn["nominees"]), f"{where}: the id space does not move"
    c = ctx.seq_nominated_read()
    assert c["n"] == len(model["consumed"]) and list(zip(c["id"].tolist(), c["pod"].tolist(), c["node"].tolist())) == model["consumed"], f"{where}: consumed rows"
    return r, model


# ---- the empty case -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 2, 12])
def test_empty_table_and_no_own_ids_equal_bs_seq_run_on_a_twin(S):
    saved = scenarios.SCALARS
    scenarios.SCALARS = NAMES12
    try:
        sc = scenarios.random_objects(4201 + S, n_nodes=70, n_groups=8, n_pods=130, n_scalars=S, n_classes=3)
    finally:
        scenarios.SCALARS = saved
    nodes, fit, groups, pods, _ = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], denied=sc["denied"], permitted=sc["permitted"])
    nodes.requested[:3] = nodes.requested[:3] // 3
    assert nodes.lanes == 4 + S
    prio = np.arange(pods.p, dtype=np.int32) % 7
    with load_ctx(bsa, nodes, fit, groups, pods) as a, load_ctx(bsa, nodes, fit, groups, pods) as b:
        b.nominated_load()
        ra, rb = a.seq_run(soa.STAGE_PREFILTER), b.seq_run_nominated(prio, None)
        for k in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "last_permitted", "released_group", "released_pods"):
            assert np.array_equal(ra[k], rb[k]), k
        for k in ("n_released", "node_picks", "node_scans"):
            assert ra[k] == rb[k], k
        assert (rb["pod_node"] >= 0).sum() > 0
        qa, qb = a.read_node_requests(), b.read_node_requests()
        assert np.array_equal(qa[0], qb[0]) and np.array_equal(qa[1], qb[1])
        assert_groups_equal(b.read_groups(), a.read_groups(), soa, f"S {S}")
        assert np.array_equal(a.seq_waiting_read(), b.seq_waiting_read())
        assert b.seq_nominated_read()["n"] == 0 and b.nominated_count() == 0


# ---- model parity, cursors on and off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cursor", ["cursors", "no-cursor"])
@pytest.mark.parametrize("seed,n,m", sns.PARITY, ids=[f"{s}-N{n}-m{m}" for s, n, m in sns.PARITY])
def test_the_pass_equals_the_model(seed, n, m, cursor, monkeypatch):
    if cursor == "no-cursor":
        monkeypatch.setenv("BS_SEQ_NO_CURSOR", "1")
    key = ("parity", seed, n, m)
    with _open(_case(key)[1]) as ctx:
        _check(ctx, key, f"seed {seed} N {n} m {m} {cursor}", flat=bool(seed & 1))


# ---- the hand-derived answers on the device -----------------------------------------------------------------------------------------------------
_KATS = sns.load_kats()


@pytest.mark.parametrize("cursor", ["cursors", "no-cursor"])
@pytest.mark.parametrize("k,S", [(i, S) for i, kat in enumerate(_KATS) for S in (0, 2) if len(kat.get("scalars", [])) <= S],
                         ids=lambda v: str(v))
def test_hand_answers_on_the_device(k, S, cursor, monkeypatch):
    if cursor == "no-cursor":
        monkeypatch.setenv("BS_SEQ_NO_CURSOR", "1")
    kat, key = _KATS[k], ("kat", k, S)
    with _open(_case(key)[1]) as ctx:
        r, model = _check(ctx, key, f"scene {kat['name']} S {S}")
        wait = ctx.seq_waiting_read()
        assumed = np.where(r["pod_node"] >= 0, r["pod_node"], wait)
        assert assumed.tolist() == kat["expect_node"], kat["why"]
        assert ctx.nominated_read()["id"].tolist() == kat["expect_rows"], kat["why"]


# ---- edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,at", [(65, (63, 64)), (129, (63, 64, 128))])
def test_nominees_on_tile_borders(n, at):
    key = ("edge", 7001, (("n_nodes", n), ("m", 7), ("first_open", 60), ("row_nodes", at)))
    scn, parts, model = _case(key)
    assert {o.node for o in scn["nominees"]} >= set(at) and model["blocked"] > 0
    with _open(parts) as ctx:
        _check(ctx, key, f"N {n} rows on {at}")


@pytest.mark.parametrize("seed", [7100, 7107])
def test_own_rows_around_the_staging_window(seed):
    key = ("edge", seed, (("n_nodes", 48), ("m", 64), ("own_pods", (63, 64, 65)), ("own_rows", (0, 1, 2))))
    model = _case(key)[2]
    assert [(i, p) for i, p, _ in model["consumed"]] == [(0, 63), (1, 64), (2, 65)]
    with _open(_case(key)[1]) as ctx:
        _check(ctx, key, f"seed {seed}")


@pytest.mark.parametrize("seed,own", [(7201, (0, 30, 77)), (7202, (0, 25, 74))])
def test_consumed_rows_around_the_compaction_window_and_a_small_cap(seed, own):
    key = ("edge", seed, (("n_nodes", 48), ("m", 1025), ("n_pods", 80), ("own_pods", own), ("own_rows", (0, 1023, 1024))))
    model = _case(key)[2]
    assert [i for i, _, _ in model["consumed"]] == [0, 1023, 1024]
    with _open(_case(key)[1]) as ctx:
        _check(ctx, key, f"seed {seed}")
        assert ctx.nominated_count() == 1022
        c = ctx.seq_nominated_read(cap=1)                                     # cap smaller than the consumed count
        assert c["n"] == 3 and c["id"].tolist() == [0] and c["pod"].tolist() == [own[0]]
        c = ctx.seq_nominated_read(cap=0)
        assert c["n"] == 3 and c["id"].size == 0


# ---- downstream ------------------------------------------------------------------------------------------------------------------------------
def test_a_preemption_plan_after_the_pass_equals_a_twin_that_removed_the_consumed_ids():
    sc, _ = pp.pdb_scene(8101, n=96, per_node=(2, 6), S=2, q=40, groups=4, share=0.0)
    rng = np.random.default_rng(8101)
    nodes, pods, P = sc["nodes"], sc["pods"], sc["pods"].p
    nodes.requested[:3] //= 2                                                  # room for the pass to place pods (the victim search works on whatever is requested)
    m = 60
    tab = dict(node=rng.integers(0, nodes.n, size=m).astype(np.uint32), priority=rng.integers(0, 6000, size=m).astype(np.int32),
               req=np.zeros((nodes.lanes, m), np.int64), req_present=np.zeros(m, np.uint32))
    tab["req"][0] = rng.integers(100, 4000, size=m)
    prio = rng.integers(0, 6000, size=P).astype(np.int32)
    own = np.full(P, capi.NOM_NONE, np.uint32)
    own_pods = rng.permutation(P)[:12]
    own[own_pods] = np.arange(12, dtype=np.uint32)
    for i, r in zip(own_pods, range(12)):                                      # an own row carries its pod's request and priority
        tab["req"][:3, r], tab["priority"][r] = pods.req[:3, i], prio[i]
    groups = groups_for(sc)
    a = bsa.Context(scalar_lanes=sc["S"], device=0)
    with a:
        a.load_nodes(nodes, sc["fit"]); a.load_groups(groups); a.load_pods(pods); a.load_bound(sc["bound"])
        a.nominated_load(tab["node"], tab["priority"], tab["req"], tab["req_present"])
        a.seq_run_nominated(prio, own)
        gone = a.seq_nominated_read()
        assert gone["n"] > 0 and a.nominated_count() == m - gone["n"]
        req, pres = a.read_node_requests()
        after = soa.Nodes(nodes.allocatable.copy(), req.copy(), nodes.allocatable_present.copy(), pres.copy(), nodes.flags.copy())
        ga = a.read_groups()
        ra = a.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=8)
        with bsa.Context(scalar_lanes=sc["S"], device=0) as b:
            b.load_nodes(after, sc["fit"]); b.load_groups(ga); b.load_pods(pods); b.load_bound(sc["bound"])
            b.nominated_load(tab["node"], tab["priority"], tab["req"], tab["req_present"])
            b.nominated_apply(remove=gone["id"])
            ta, tb = a.nominated_read(), b.nominated_read()
            for k in ta:
                assert np.array_equal(ta[k], tb[k]), k
            rb = b.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=8)
        for k in ra:
            assert np.array_equal(ra[k], rb[k]), k
        assert (ra["node"] >= 0).sum() > 0


def test_expire_after_the_pass_and_a_second_pass_that_names_a_consumed_id():
    key = ("parity", 5207, 130, 64)
    scn, parts, model = _case(key)
    with _open(parts) as ctx:
        _check(ctx, key, "first pass")
        nodes, groups, wait = snr.end_state_soa(model, scn["sc"], soa, dict(parts[4]))
        assert (wait >= 0).sum() > 0
        before = _state(ctx)
        assert model["consumed"], "the scene consumes rows"
        with pytest.raises(capi.BsError) as e:                                 # a consumed id is dead exactly as after bs_nominated_apply
            ctx.seq_run_nominated(scn["priority"], scn["own_id"])
        assert e.value.status == INVALID
        _same_state(before, _state(ctx), "refused second pass")
        assert np.array_equal(ctx.seq_waiting_read(), wait), "a refused pass leaves the window of the last one open"
        st = sx.State(nodes.requested, nodes.requested_present, groups.matched, groups.flags, wait)
        exp = sx.expire(st, parts[3], all=True, deny=True)
        got = ctx.seq_expire(all=True, deny=True)
        for k in ("n_groups", "n_pods"):
            assert got[k] == exp[k], k
        for k in ("group", "group_pods", "group_earlier", "pod", "node"):
            assert np.array_equal(got[k], exp[k]), k
        req, pres = ctx.read_node_requests()
        assert np.array_equal(req, st.requested) and np.array_equal(pres, st.requested_present)
        g = ctx.read_groups()
        assert np.array_equal(g.matched, st.matched) and np.array_equal(g.flags, st.flags)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_nothing_changes():
    key = ("parity", 5201, 130, 64)
    scn, parts, model = _case(key)
    prio, own, P = scn["priority"], scn["own_id"], len(scn["priority"])
    with _open(parts) as ctx:
        before = _state(ctx)

        def refused(status, where, *a, **kw):
            with pytest.raises(capi.BsError) as e:
                ctx.seq_run_nominated(*a, **kw)
            assert e.value.status == status, (where, str(e.value))
            _same_state(before, _state(ctx), where)
            with pytest.raises(capi.BsError) as e2:
                ctx.seq_nominated_read()
            assert e2.value.status == STATE, where

        refused(INVALID, "no PREFILTER", prio, own, stages=soa.STAGE_FILTER)
        refused(INVALID, "FILTER", prio, own, stages=soa.STAGE_PREFILTER | soa.STAGE_FILTER)
        refused(INVALID, "FILTER + deny", prio, own, stages=soa.STAGE_PREFILTER | soa.STAGE_FILTER | soa.BATCH_FILTER_DENY)
        refused(INVALID, "deny without FILTER", prio, own, stages=soa.STAGE_PREFILTER | soa.BATCH_FILTER_DENY)
        refused(INVALID, "p too small", prio, own, p=P - 1)
        refused(INVALID, "p too large", prio, own, p=P + 1)
        refused(INVALID, "NULL priority", None, own)
        bad = own.copy()
        bad[np.nonzero(own == capi.NOM_NONE)[0][0]] = len(scn["nominees"])
        refused(INVALID, "unknown own id", prio, bad)
        twice = own.copy()
        twice[np.nonzero(own == capi.NOM_NONE)[0][0]] = own[own != capi.NOM_NONE][0]
        refused(INVALID, "an own id named by two pods", prio, twice)
        live = own[own != capi.NOM_NONE]
        ctx.nominated_apply(remove=live[:1])
        before = _state(ctx)
        refused(INVALID, "dead own id", prio, own)
        tab_before = _state(ctx)
        ctx.apply_node_deltas([capi.NodeDelta(kind=capi.DELTA_REMOVE, index=parts[0].n - 1)])
        def rest(c):                                                            # (bs_nominated_read refuses the stale count too)
            req, pres = c.read_node_requests()
            g = c.read_groups()
            return dict(req=req, pres=pres, matched=g.matched.copy(), flags=g.flags.copy(), sc=g.status_scheduled.copy(), ids=c.nominated_ids(), rows=c.nominated_count())

        before = rest(ctx)
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_nominated(prio, None)
        assert e.value.status == STATE
        _same_state(before, rest(ctx), "stale node count")
        ctx.nominated_nodes_apply([capi.DELTA_REMOVE], [parts[0].n - 1])         # the table follows the surgery: its rows are as they were, but for the node's
        after = _state(ctx)
        assert np.array_equal(after["t_id"], tab_before["t_id"][tab_before["t_node"] != parts[0].n - 1])
    nodes, fit, groups, pods = parts[:4]
    def plain(c):
        req, pres = c.read_node_requests()
        g = c.read_groups()
        return dict(req=req, pres=pres, matched=g.matched.copy(), flags=g.flags.copy(), sc=g.status_scheduled.copy())

    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:                       # no table at all
        before = plain(ctx)
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_nominated(prio, None)
        assert e.value.status == STATE
        _same_state(before, plain(ctx), "no table")
        ctx.nominated_load(*[parts[5][k] for k in ("node", "priority", "req", "req_present")])
        ctx.reduce_external(True)                                              # an external-reduce context
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_nominated(prio, own)
        assert e.value.status == STATE
        ctx.reduce_external(False)
        _same_state(dict(before, ids=len(scn["nominees"]), rows=len(scn["nominees"])), dict(plain(ctx), ids=ctx.nominated_ids(), rows=ctx.nominated_count()), "external reduce")
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:                       # a sharded context
        before = plain(ctx)
        ctx.nominated_load()
        ctx.set_shard(0, 2)
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_nominated(prio, None)
        assert e.value.status == STATE
        ctx.set_shard(0, 1)
        _same_state(before, plain(ctx), "sharded")
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:                     # what bs_seq_run refuses, with its code
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_nominated(prio, None, p=P)
        assert e.value.status == STATE
    lib = capi.load_library()
    assert lib.bs_seq_run_nominated(None, 1, 0, None, None, None) == INVALID and lib.bs_seq_nominated_read(None, 0, None, None, None, None) == INVALID


def test_the_read_call_follows_the_last_pass():
    key = ("parity", 5203, 48, 7)
    scn, parts, _ = _case(key)
    with _open(parts) as ctx:
        with pytest.raises(capi.BsError) as e:
            ctx.seq_nominated_read()
        assert e.value.status == STATE
        _check(ctx, key, "pass")
        ctx.seq_run(soa.STAGE_PREFILTER)                                        # the last pass is bs_seq_run now
        with pytest.raises(capi.BsError) as e:
            ctx.seq_nominated_read()
        assert e.value.status == STATE
