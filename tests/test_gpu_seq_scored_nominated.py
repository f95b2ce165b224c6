"""GPU tests of bs_seq_run_scored_nominated (include/bsched.h, rule SP, D8, SP1, SP2; csrc/bs_seq.hpp, seq_pick_scored<TS, true> and
k_seq_sp<TS>): the sequential pass under rules S and P at once against the object-level model tests/seq_scored_nominated_ref.py, bit for bit —
every output, bs_seq_score_read, bs_seq_nominated_read, the surviving table, the node requests and group state the pass leaves; the two
reductions on twin contexts; every weight triple around a tile border with rows on both sides; the geometry of the tile walk with rows on
it; row chains and int64 extremes; the hand-derived answers; one real cycle behind the pass; the nominating cycle end to end; every refusal.
Scenes are small (1 to 513 nodes, at most 200 pods) except the one that needs two tile walks (32 838 nodes, six pods); models are computed
once per scene.  tests/test_seq_scored_nominated_cpu.py asserts that this scene set meets every hazard letter of the model."""
import functools
import importlib

import numpy as np
import pytest

import bound_apply_ref as bar
import naive_ref as nv
import seq_expire_ref as sx
import seq_nominated_ref as snr
import seq_nominated_scenes as sns
import seq_scored_nominated_ref as spr
import seq_scored_nominated_scenes as sps
import seq_scored_nominated_soa as spsoa
import seq_scored_scenes as sss
import seq_soa_ref as ssoa
import wait_ref as wr
from test_gpu_bound_bind import B, three_valued
from test_gpu_parity import load_ctx
from test_gpu_seq import assert_groups_equal
from test_gpu_wait import W

bsa = importlib.import_module("batch-scheduler_amd")
capi, soa = bsa.capi, bsa.soa
pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -4
PF = soa.STAGE_PREFILTER
OUTPUTS = ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods")
GI, I64_MAX = sss.GI, sss.I64_MAX
KATS = sps.load_kats()


def chain_scene():
    """four nodes.  Node 1 (empty) carries a chain of five rows with priorities 3, 10, 7, 10, 20 around the pods' 7, the middle one owned by
    pod 1; node 2 a row with a negative lane; node 3 two rows whose cpu lanes are 2^63 - 1 and 2^40 (their sum wraps).  Pod 2 is the very
    next pod behind the consume of pod 1's row.  The model decides what is expected."""
    nodes = [sss._node(4000, 8 * GI, 2500, 0), sss._node(4000, 8 * GI, 0, 0), sss._node(4000, 8 * GI, 3000, 0), sss._node(4000, 8 * GI, 1000, 0)]
    R = lambda cpu, mem=0: nv.Resource(cpu, mem, 0, 1, None)
    rows = [snr.Nominee(0, 1, 3, R(500)), snr.Nominee(1, 1, 10, R(500)), snr.Nominee(2, 1, 7, R(1000)), snr.Nominee(3, 1, 10, R(500)), snr.Nominee(4, 1, 20, R(500)),
            snr.Nominee(5, 2, 10, R(-1000)), snr.Nominee(6, 3, 10, R(I64_MAX)), snr.Nominee(7, 3, 10, R(1 << 40)), snr.Nominee(8, 0, 8, R(0, I64_MAX))]
    reqs = [1500, 1000, 1500, 1000, 500, 2500, 500, 500]
    prio = [7, 7, 7, 12, 3, 30, 10, 7]
    pods = [nv.Pod(f"uid{i}", None, {"cpu": c, "memory": GI if i & 1 else 0}) for i, c in enumerate(reqs)]
    own = np.full(len(pods), snr.NOM_NONE, np.uint32)
    own[1] = 2
    sc = dict(nodes=nodes, cache={}, pods=pods, names=[], n_classes=1, denied=set(), permitted=set())
    return dict(sc=sc, names=[], priority=np.array(prio, np.int32), own_id=own, nominees=rows, rowless=None, weights=(1, 0, 1))


@functools.lru_cache(maxsize=None)
def _case(key):
    """(scene, its SoA): computed once, never changed"""
    kind = key[0]
    if kind == "parity":
        scn = sps.parity_scene(*key[1:])
    elif kind == "lean":
        scn = sps.lean_scene(*key[1:])
    elif kind == "kat":
        scn = sps.kat_scene(KATS[key[1]])
    elif kind == "border":
        scn = sps.border_scene(key[1], key[2])
    elif kind == "nom":
        scn = dict(sns.parity_scene(*key[1:]), weights=(0, 0, 0))
    else:
        scn = dict(walks=sps.walks_scene, waves=sps.waves_scene, chain=chain_scene)[kind]()
    return scn, sps.to_soa(scn)


@functools.lru_cache(maxsize=None)
def _model(key, weights=None):
    return sps.model(_case(key)[0], weights)


def _open(key, rows=True):
    nodes, fit, groups, pods, _, tab = _case(key)[1]
    ctx = load_ctx(bsa, nodes, fit, groups, pods)
    if rows:
        ctx.nominated_load(tab["node"], tab["priority"], tab["req"], tab["req_present"])
    return ctx


def _state(ctx):
    """everything resident that can be read: node requests, groups, the table with its id space"""
    req, pres = ctx.read_node_requests()
    g = ctx.read_groups()
    t = ctx.nominated_read()
    return dict(req=req, pres=pres, matched=g.matched.copy(), flags=g.flags.copy(), sc=g.status_scheduled.copy(), cls=g.cls.copy(), mr=g.min_resources.copy(),
                occ=g.occupied_by.copy(), ids=ctx.nominated_ids(), **{"t_" + k: v.copy() for k, v in t.items()})


def _same_state(a, b, where):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{where}: {k} differs"


def _check(ctx, key, where, weights=None, flat=False):
    """one bs_seq_run_scored_nominated on ctx against the model of scene `key`"""
    (scn, parts), model = _case(key), _model(key, weights)
    r = ctx.seq_run_scored_nominated(scn["weights"] if weights is None else weights, scn["priority"], scn["own_id"], flat=flat)
    for k in OUTPUTS:
        assert r[k].tolist() == list(model[k]), f"{where}: {k}"
    assert not r["last_permitted"].any()
    s = ctx.seq_score_read()
    assert s["total"].tolist() == model["total"], f"{where}: total"
    assert s["n_fit"].tolist() == model["n_fit"], f"{where}: n_fit"
    nodes, groups, wait = spr.end_state_soa(model, scn["sc"], soa, dict(parts[4]))
    req, pres = ctx.read_node_requests()
    assert np.array_equal(req, nodes.requested), f"{where}: node requests after the pass (no row in them)"
    assert np.array_equal(pres, nodes.requested_present), f"{where}: node request keys"
    assert_groups_equal(ctx.read_groups(), groups, soa, where)
    assert np.array_equal(ctx.seq_waiting_read(), wait), f"{where}: the pods still waiting at Permit"
    assumed = np.where(r["pod_node"] >= 0, r["pod_node"], wait)
    assert assumed.tolist() == model["assumed"], f"{where}: the node every pod was assumed on"
    left = spr.objects_to_rows(model["nominees"], scn["names"])
    got = ctx.nominated_read()
    for k in ("id", "node", "priority", "req", "req_present"):
        assert np.array_equal(got[k], left[k]), f"{where}: surviving table, {k}"
    assert ctx.nominated_ids() == len(scn["nominees"]), f"{where}: the id space does not move"
    c = ctx.seq_nominated_read()
    assert c["n"] == len(model["consumed"]) and list(zip(c["id"].tolist(), c["pod"].tolist(), c["node"].tolist())) == model["consumed"], f"{where}: consumed rows"
    return r, model, (nodes, groups, wait)


# ---- model parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sps.PARITY)), ids=[f"{s}-N{n}-m{m}-S{S}" for s, n, m, S in sps.PARITY])
def test_the_pass_equals_the_model(i):
    key = ("parity",) + sps.PARITY[i]
    with _open(key) as ctx:
        _check(ctx, key, str(key), flat=bool(i & 1))


@pytest.mark.parametrize("i", range(len(sps.LEAN)), ids=[f"{s}-N{n}-m{m}-S{S}" for s, n, m, S in sps.LEAN])
def test_the_pass_equals_the_model_in_the_lean_form(i):
    """5, 9 and 12 scalar lanes: the kernel keeps no row sums, it walks a node's chain once per lane the pod asks for.  The rows carry scalar
    lanes, and on the model a row's scalar sum and a key only the row brings each decide a node"""
    key = ("lean",) + sps.LEAN[i]
    hz = _model(key)["hazards"]
    assert hz["s"] >= 1 and hz["i"] >= 1, hz
    with _open(key) as ctx:
        _check(ctx, key, str(key), flat=bool(i & 1))


# ---- SP1 and SP2 on twin contexts ------------------------------------------------------------------------------------------------------------------
def _twins_equal(a, b, ra, rb, where):
    for k in OUTPUTS + ("last_permitted",):
        assert np.array_equal(ra[k], rb[k]), f"{where}: {k}"
    for k in ("n_released", "node_picks", "node_scans"):
        assert ra[k] == rb[k], f"{where}: {k}"
    _same_state(_state(a), _state(b), where)
    assert_groups_equal(b.read_groups(), a.read_groups(), soa, where)
    assert np.array_equal(a.seq_waiting_read(), b.seq_waiting_read()), where
    assert a.find_max_pg() == b.find_max_pg(), where


@pytest.mark.parametrize("key", [("nom",) + sns.PARITY[1], ("nom",) + sns.PARITY[5], ("nom",) + sns.PARITY[11], ("lean",) + sps.LEAN[2]], ids=str)
def test_sp1_zero_weights_equal_bs_seq_run_nominated_on_a_twin(key):
    scn = _case(key)[0]
    with _open(key) as a, _open(key) as b:
        ra = a.seq_run_nominated(scn["priority"], scn["own_id"])
        rb = b.seq_run_scored_nominated((0, 0, 0), scn["priority"], scn["own_id"])
        _twins_equal(a, b, ra, rb, str(key))
        ca, cb = a.seq_nominated_read(), b.seq_nominated_read()
        assert ca["n"] == cb["n"] and all(np.array_equal(ca[k], cb[k]) for k in ("id", "pod", "node"))
        assert (rb["pod_node"] >= 0).sum() > 0 and not b.seq_score_read()["total"].any()
        assert b.seq_score_read()["n_fit"].tolist() == _model(key, (0, 0, 0))["n_fit"]


@pytest.mark.parametrize("i,weights", [(4, (1, 0, 1)), (7, (0, 1, 0)), (14, (3, 2, 1)), (2, (0, 0, 1))], ids=str)
def test_sp2_an_empty_table_and_no_own_ids_equal_bs_seq_run_scored_on_a_twin(i, weights):
    key = ("parity",) + sps.PARITY[i]
    nodes, fit, groups, pods, _, _ = _case(key)[1]
    prio = np.arange(pods.p, dtype=np.int32) % 7
    with load_ctx(bsa, nodes, fit, groups, pods) as a, load_ctx(bsa, nodes, fit, groups, pods) as b:
        a.nominated_load()
        b.nominated_load()                                                       # empty but loaded
        ra, rb = a.seq_run_scored(weights), b.seq_run_scored_nominated(weights, prio, None)
        _twins_equal(a, b, ra, rb, str(key))
        sa, sb = a.seq_score_read(), b.seq_score_read()
        assert np.array_equal(sa["total"], sb["total"]) and np.array_equal(sa["n_fit"], sb["n_fit"]) and sa["total"].any()
        assert b.seq_nominated_read()["n"] == 0 and b.nominated_count() == 0


# ---- every weight triple around a tile border, a row on each side ------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", sss.WEIGHTS, ids=str)
@pytest.mark.parametrize("n", [65, 8 * 64 + 1])
def test_every_weight_triple_around_a_tile_border(n, weights):
    key = ("border", n, weights)
    assert _model(key)["hazards"]["h"] >= 1
    with _open(key) as ctx:
        _check(ctx, key, f"N {n} {weights}")


# ---- geometry by construction ------------------------------------------------------------------------------------------------------------------------
def test_two_tile_walks_a_row_decides_the_tie_between_them():
    key, W_ = ("walks",), sss.WALK
    with _open(key) as ctx:
        r, model, _ = _check(ctx, key, "walks")
        assert r["pod_node"].tolist()[1] == W_ and r["pod_node"].tolist()[3] == W_ and r["pod_node"].tolist()[5] == W_ - 1, "the row keeps 32 767 from priority 5; priority 20 takes it"
        assert model["n_fit"] == [2, 2, 2, 2, 2, 3]


def test_a_row_on_the_better_of_two_nodes_one_lane_sees():
    key = ("waves",)
    with _open(key) as ctx:
        r, _, _ = _check(ctx, key, "waves")
        assert r["pod_node"].tolist() == [66 * 64 + 1, 66 * 64 + 9, 65 * 64 + 5, 64 * 64 + 5, 65 * 64 + 5, 66 * 64 + 1]


# ---- chains and extremes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1, 0, 1), (0, 1, 0)], ids=str)
def test_a_chain_of_five_rows_an_own_row_inside_it_and_int64_extremes(weights):
    key = ("chain",)
    model = _model(key, weights)
    assert (2, 1) in [(i, p) for i, p, _ in model["consumed"]], "pod 1 is assumed and its row, the middle of the chain, is consumed"
    assert model["hazards"]["k"] >= 1 and model["hazards"]["h"] >= 1 and sum(1 for a in model["assumed"] if a >= 0) >= 5, model["hazards"]
    with _open(key) as ctx:
        _check(ctx, key, f"chain {weights}", weights=weights)


def test_a_consumed_row_frees_its_node_for_the_very_next_pod():
    key = ("kat", [k["name"] for k in KATS].index("d"))
    assert _model(key)["hazards"]["d"] >= 1
    with _open(key) as ctx:
        r, _, _ = _check(ctx, key, "hand scene d")
        assert r["pod_node"].tolist() == [0, 0]


# ---- the hand-derived answers on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(KATS)), ids=[k["name"] for k in KATS])
def test_hand_answers_on_the_device(k):
    kat, key = KATS[k], ("kat", k)
    with _open(key) as ctx:
        r, _, _ = _check(ctx, key, f"scene {kat['name']}")
        assert r["pod_node"].tolist() == kat["expect_node"], kat["why"]
        s = ctx.seq_score_read()
        assert s["total"].tolist() == kat["expect_total"] and s["n_fit"].tolist() == kat["expect_n_fit"], kat["why"]
        assert ctx.nominated_read()["id"].tolist() == kat["expect_rows"], kat["why"]


# ---- one real cycle behind the pass ------------------------------------------------------------------------------------------------------------------
CYCLE = ("parity",) + sps.PARITY[20]                                            # 130 nodes, 64 rows, four scalar lanes, gangs


def test_expire_park_and_bind_behind_the_pass(orc):
    scn, parts = _case(CYCLE)
    pods, S, N, G = parts[3], parts[0].lanes - 4, parts[0].n, parts[2].g
    rng = np.random.default_rng(37)
    with _open(CYCLE) as ctx:
        r, model, (nodes, groups, wait) = _check(ctx, CYCLE, "the pass")
        waiting_groups = sorted({int(pods.group[i]) for i in np.nonzero(wait >= 0)[0]})
        assert len(waiting_groups) >= 2 and (r["pod_node"] >= 0).sum() >= 2, "gangs that missed their quorum, and placed pods"
        st = sx.State(nodes.requested, nodes.requested_present, groups.matched, groups.flags, wait)
        g0 = waiting_groups[0]
        exp = sx.expire(st, pods, groups=[g0], deny=True)
        got = ctx.seq_expire(groups=[g0], deny=True)
        for k in ("n_groups", "n_pods"):
            assert got[k] == exp[k], k
        for k in ("group", "group_pods", "group_earlier", "pod", "node"):
            assert np.array_equal(got[k], exp[k]), k
        assert exp["n_pods"] >= 1
        ctx.wait_load()
        w = W(ctx, soa, orc, st, groups, wr.load(N, G, S), pods, window=True)
        w.check("after the expire")
        pk = w.park("park")
        assert pk["n"] == int((wait >= 0).sum()) - exp["n_pods"] and np.all(ctx.seq_waiting_read() == -1)
        bound = three_valued(rng, N, 30, S)
        ctx.load_bound(bound)
        pl = np.nonzero(r["pod_node"] >= 0)[0]
        b = B(ctx, soa, bar.Table(bound, S, N), w.tab, N, G, pods=pods, pod_node=r["pod_node"].astype(np.int32), wait_node=st.wait_node, window=True)
        out = b.bind("bind the placed pods", (), pl, rng.integers(0, 3, pl.size).astype(np.int32), rng.integers(0, 3, pl.size).astype(np.int64))
        assert np.array_equal(out["node"], r["pod_node"][pl].astype(np.uint32)), "a placed pod brings the node the pass chose"


def test_a_plain_pass_behind_it_equals_the_oracle_from_that_state(orc):
    fit, pods = _case(CYCLE)[1][1], _case(CYCLE)[1][3]
    with _open(CYCLE) as ctx:
        _, model, (nodes, groups, _) = _check(ctx, CYCLE, "the pass")
        s2 = orc.seq_replay(nodes, fit, groups, pods, PF, leader=model["pf_leader"][-1])
        r2 = ctx.seq_run(PF)
        for k in OUTPUTS:
            assert np.array_equal(r2[k], s2[k]), f"the plain pass: {k}"
        req, pres = ctx.read_node_requests()
        assert np.array_equal(req, s2["nodes"].requested) and np.array_equal(pres, s2["nodes"].requested_present)
        assert_groups_equal(ctx.read_groups(), s2["groups"], soa, "the plain pass")
        assert (r2["pod_node"] >= 0).sum() + (ctx.seq_waiting_read() >= 0).sum() > 0, "the second pass placed pods"
        for read in (ctx.seq_score_read, ctx.seq_nominated_read):                 # after any other pass the two reads behave as they do today
            with pytest.raises(capi.BsError) as e:
                read()
            assert e.value.status == STATE


# ---- the nominating cycle, end to end ------------------------------------------------------------------------------------------------------------------
def _cycle_scene():
    """six nodes of 4000 m, each with eight bound pods of 400 m (free: 800 m); the bound pods of nodes 4 and 5 have the lowest priority.  Queue:
    six small pods (600 m, priority 0) IN FRONT of two preemptors (2000 m, priority 100); nobody is grouped."""
    nodes = [sss._node(4000, 8 * GI, 3200, 0, pods=110) for _ in range(6)]
    for info in nodes:
        info.pod_count = 8
    pods = [nv.Pod(f"uid{i}", None, {"cpu": 600}) for i in range(6)] + [nv.Pod(f"uid{6 + i}", None, {"cpu": 2000}) for i in range(2)]
    sc = dict(nodes=nodes, cache={}, pods=pods, names=[], n_classes=1, denied=set(), permitted=set())
    b = 48
    req = np.zeros((4, b), np.int64)
    req[0], req[3] = 400, 1
    node = np.repeat(np.arange(6, dtype=np.uint32), 8)
    bound = soa.Bound(node, np.where(node >= 4, -10, 0).astype(np.int32), np.arange(b, dtype=np.int64), np.full(b, -1, np.int32), req, np.zeros(b, np.uint32))
    return sc, bound, np.array([0] * 6 + [100] * 2, np.int32)


def test_the_nominating_cycle_end_to_end(orc):
    sc, bound, prio = _cycle_scene()
    nodes, fit, groups, pods, _ = sss.to_soa(sc)
    weights = (1, 0, 0)
    with load_ctx(bsa, nodes, fit, groups, pods) as a, load_ctx(bsa, nodes, fit, groups, pods) as b:
        plans = []
        for ctx in (a, b):
            ctx.load_bound(bound)
            ctx.nominated_load()
            plans.append(ctx.preempt_commit([6, 7], prio[6:], victim_cap=8, apply=True, nominate=True, clear_lower=True))
        plan = plans[0]
        freed = plan["node"].tolist()
        assert all(k >= 0 for k in freed) and len(set(freed)) == 2 and np.array_equal(plans[0]["node"], plans[1]["node"]), "both preemptors hold a node of their own"
        own = np.full(pods.p, capi.NOM_NONE, np.uint32)
        own[6:] = plan["nominated_id"]
        assert (own[6:] != capi.NOM_NONE).all() and a.nominated_count() == 2
        # the model, from the state the plan left on the device
        req, pres = a.read_node_requests()
        after = soa.Nodes(nodes.allocatable.copy(), req.copy(), nodes.allocatable_present.copy(), pres.copy(), nodes.flags.copy())
        assert all(int(req[0, k]) == 3200 - 3 * 400 for k in freed), "three victims of 400 m left each chosen node"
        ch = spsoa.ScoredNominatedChoice(a.nominated_read(), prio, own, weights, pods.p)
        model = ssoa.seq_pass(orc, after, fit, groups, pods, -1, ch)
        assert model["pod_node"][6:].tolist() == freed, "on the model every preemptor lands on the node that was emptied for it"
        assert sorted(ch.consumed) == [(int(own[6]), 6, freed[0]), (int(own[7]), 7, freed[1])] and not set(model["pod_node"][:6].tolist()) & set(freed)
        # the pass under both rules
        r = a.seq_run_scored_nominated(weights, prio, own)
        for k in OUTPUTS:
            assert np.array_equal(r[k], model[k]), k
        s = a.seq_score_read()
        assert np.array_equal(s["total"], ch.total) and np.array_equal(s["n_fit"], ch.n_fit)
        req2, pres2 = a.read_node_requests()
        assert np.array_equal(req2, model["nodes"].requested) and np.array_equal(pres2, model["nodes"].requested_present)
        c = a.seq_nominated_read()
        assert list(zip(c["id"].tolist(), c["pod"].tolist(), c["node"].tolist())) == sorted(ch.consumed) and a.nominated_count() == 0
        assert r["pod_node"][6:].tolist() == freed and not set(r["pod_node"][:6].tolist()) & set(freed), "no lower-priority pod took the freed room"
        # ... and the scored pass that does not see the table gives that room away on the same scene
        rb = b.seq_run_scored(weights)
        assert set(freed) <= set(rb["pod_node"][:6].tolist()) and rb["pod_node"][6:].tolist() == [-1, -1], "small pods scored into the freed room, the preemptors find it full"


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_both_parents_and_nothing_changes():
    key = ("parity",) + sps.PARITY[20]
    scn, parts = _case(key)
    prio, own, P, w = scn["priority"], scn["own_id"], len(scn["priority"]), (1, 0, 1)
    lib = capi.load_library()
    with _open(key) as ctx:
        before = _state(ctx)

        def refused(status, where, *a, **kw):
            with pytest.raises(capi.BsError) as e:
                ctx.seq_run_scored_nominated(*a, **kw)
            assert e.value.status == status, (where, str(e.value))
            _same_state(before, _state(ctx), where)
            for read in (ctx.seq_nominated_read, ctx.seq_score_read):           # no pass has run: both reads refuse as before
                with pytest.raises(capi.BsError) as e2:
                    read()
                assert e2.value.status == STATE, where

        # what bs_seq_run_nominated refuses
        refused(INVALID, "no PREFILTER", w, prio, own, stages=soa.STAGE_FILTER)
        refused(INVALID, "FILTER", w, prio, own, stages=PF | soa.STAGE_FILTER)
        refused(INVALID, "FILTER + deny", w, prio, own, stages=PF | soa.STAGE_FILTER | soa.BATCH_FILTER_DENY)
        refused(INVALID, "deny without FILTER", w, prio, own, stages=PF | soa.BATCH_FILTER_DENY)
        refused(INVALID, "p too small", w, prio, own, p=P - 1)
        refused(INVALID, "p too large", w, prio, own, p=P + 1)
        refused(INVALID, "NULL priority", w, None, own)
        bad = own.copy()
        bad[np.nonzero(own == capi.NOM_NONE)[0][0]] = len(scn["nominees"])
        refused(INVALID, "unknown own id", w, prio, bad)
        twice = own.copy()
        twice[np.nonzero(own == capi.NOM_NONE)[0][0]] = own[own != capi.NOM_NONE][0]
        refused(INVALID, "an own id named by two pods", w, prio, twice)
        # what bs_seq_run_scored refuses
        refused(INVALID, "NULL score", None, prio, own)
        for j in range(3):
            big = [1, 1, 1]
            big[j] = capi.SCORE_WEIGHT_MAX + 1
            refused(INVALID, f"weight {j} of 65 537", big, prio, own)
            refused(INVALID, f"weight {j} of 65 537, flat", big, prio, own, flat=True)
        for where, on, off in (("a sharded context", lambda: ctx.set_shard(0, 2), lambda: ctx.set_shard(0, 1)),
                               ("an external-reduce context", lambda: ctx.reduce_external(True), lambda: ctx.reduce_external(False))):
            on()                                                                 # (the table's own reads are single-rank only: compare once it is off again)
            with pytest.raises(capi.BsError) as e:
                ctx.seq_run_scored_nominated(w, prio, own)
            assert e.value.status == STATE, where
            off()
            _same_state(before, _state(ctx), where)
        live = own[own != capi.NOM_NONE]
        ctx.nominated_apply(remove=live[:1])
        before = _state(ctx)
        refused(INVALID, "dead own id", w, prio, own)
        # a good pass, then a refused one: the good one stays readable
        keep = own.copy()
        keep[own == live[0]] = capi.NOM_NONE
        ctx.seq_run_scored_nominated((capi.SCORE_WEIGHT_MAX,) * 3, prio, keep)   # the largest weights are fine
        s0, c0 = ctx.seq_score_read(), ctx.seq_nominated_read()
        assert int(s0["total"].max()) < 1 << 32 and c0["n"] > 0
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_scored_nominated((0, 0, 65537), prio, None)
        assert e.value.status == INVALID
        s1, c1 = ctx.seq_score_read(), ctx.seq_nominated_read()
        assert np.array_equal(s0["total"], s1["total"]) and np.array_equal(s0["n_fit"], s1["n_fit"]) and np.array_equal(c0["id"], c1["id"])
        with pytest.raises(capi.BsError) as e:                                   # a consumed id is dead
            ctx.seq_run_scored_nominated(w, prio, keep)
        assert e.value.status == INVALID
        # a stale node count
        ctx.apply_node_deltas([capi.NodeDelta(kind=capi.DELTA_REMOVE, index=parts[0].n - 1)])
        req0, pres0 = ctx.read_node_requests()
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_scored_nominated(w, prio, None)
        assert e.value.status == STATE
        req1, pres1 = ctx.read_node_requests()
        assert np.array_equal(req0, req1) and np.array_equal(pres0, pres1)
    nodes, fit, groups, pods = parts[:4]
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:                       # no table at all
        req0, _ = ctx.read_node_requests()
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_scored_nominated(w, prio, None)
        assert e.value.status == STATE and np.array_equal(req0, ctx.read_node_requests()[0])
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:                     # what bs_seq_run refuses, with its code
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_scored_nominated(w, prio, None, p=P)
        assert e.value.status == STATE
    o, sc_ = capi.SeqOut(), capi.SeqScore(1, 0, 1)
    assert lib.bs_seq_run_scored_nominated(None, 1, 0, None, None, capi.C.byref(sc_), capi.C.byref(o)) == INVALID
