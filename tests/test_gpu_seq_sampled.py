"""GPU tests of the two sampled passes (include/bsched.h, rule F, D9, F1 to F3; csrc/bs_seq.hpp, seq_pick_sampled, k_seq_sampled<TS> and
k_seq_sampled_nom<TS>): bs_seq_run_scored_sampled and bs_seq_run_scored_nominated_sampled against the object-level model
tests/seq_sampled_ref.py, bit for bit — every output, bs_seq_score_read, bs_seq_sample_read, the node requests and group state the pass leaves
and, under rule SP, the surviving table and the consumed rows.  The grid: N in {1, 63, 64, 65, 128, 129, 511, 512, 513, 1025} (a slot of the
walk is 64 nodes, a round 512), every distinct cursor of {0, 1, 63, 64, N - 1, N, N + 7}, K in {1, 2, 64, 0, N, N + 1}; K around a candidate
set of known size; every lane count that takes another path; F1 on twin contexts; F2; tiles the bounds exclude; the Filter stage; the
cursor chained across two passes; one real cycle behind the pass; every refusal; the flat twins.  Scenes are small (at most 60 pods) and
models are computed once per case.  tests/test_seq_sampled_cpu.py asserts that these very cases meet every hazard letter of the model."""
import importlib

import numpy as np
import pytest

import bound_apply_ref as bar
import seq_expire_ref as sx
import seq_sampled_ref as smr
import seq_sampled_scenes as sms
import seq_sampled_soa as smsoa
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
PF, FILTER, DENY = soa.STAGE_PREFILTER, soa.STAGE_PREFILTER | soa.STAGE_FILTER, soa.STAGE_PREFILTER | soa.STAGE_FILTER | soa.BATCH_FILTER_DENY
OUTPUTS = ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods", "last_permitted")
KATS = sms.load_kats()


def _open(case):
    nodes, fit, groups, pods, _, tab = sms.to_soa(sms.split(case)[0])
    ctx = load_ctx(bsa, nodes, fit, groups, pods)
    if tab is not None:
        ctx.nominated_load(tab["node"], tab["priority"], tab["req"], tab["req_present"])
    return ctx


def _state(ctx, table):
    """everything resident that can be read: node requests, groups and, where one is loaded, the nominated-pod table with its id space"""
    req, pres = ctx.read_node_requests()
    g = ctx.read_groups()
    out = dict(req=req, pres=pres, matched=g.matched.copy(), flags=g.flags.copy(), sc=g.status_scheduled.copy(), cls=g.cls.copy(), mr=g.min_resources.copy(),
               occ=g.occupied_by.copy())
    if table:
        out.update(ids=ctx.nominated_ids(), **{"t_" + k: v.copy() for k, v in ctx.nominated_read().items()})
    return out


def _same_state(a, b, where):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{where}: {k} differs"


def _run(ctx, case, flat=False, sample=None, weights=None):
    """the sampled pass of a case on ctx (sample / weights override the case's)"""
    key, smp, w, flt = sms.split(case)
    scn = sms.scene(case)
    smp, w = (smp if sample is None else sample), (w if weights is None else weights)
    if scn["nominees"] is None:
        return ctx.seq_run_scored_sampled(w, smp, stages=FILTER if flt else PF, flat=flat)
    return ctx.seq_run_scored_nominated_sampled(w, smp, scn["priority"], scn["own_id"], flat=flat)


def _check(ctx, case, flat=False):
    """one sampled pass on ctx against the object model of the case"""
    where = str(case)
    key = sms.split(case)[0]
    scn, parts, model = sms.scene(case), sms.to_soa(key), sms.model(case)
    r = _run(ctx, case, flat)
    for k in OUTPUTS:
        assert r[k].tolist() == list(model[k]), f"{where}: {k}"
    s = ctx.seq_score_read()
    assert s["total"].tolist() == model["total"], f"{where}: total"
    assert s["n_fit"].tolist() == model["n_fit"], f"{where}: n_fit (the candidates kept)"
    c = ctx.seq_sample_read()
    assert c["start"].tolist() == model["start"], f"{where}: the cursor every walk began at"
    assert c["visited"].tolist() == model["visited"], f"{where}: the nodes every walk visited"
    assert c["next_start"] == model["next_start"], f"{where}: the cursor behind the last pod"
    nodes, groups, wait = smr.end_state_soa(model, scn["sc"], soa, dict(parts[4]))
    req, pres = ctx.read_node_requests()
    assert np.array_equal(req, nodes.requested), f"{where}: node requests after the pass"
    assert np.array_equal(pres, nodes.requested_present), f"{where}: node request keys"
    assert_groups_equal(ctx.read_groups(), groups, soa, where)
    assert np.array_equal(ctx.seq_waiting_read(), wait), f"{where}: the pods still waiting at Permit"
    assumed = np.where(r["pod_node"] >= 0, r["pod_node"], wait)
    assert assumed.tolist() == model["assumed"], f"{where}: the node every pod was assumed on"
    if scn["nominees"] is not None:
        left = smr.objects_to_rows(model["nominees"], scn["names"])
        got = ctx.nominated_read()
        for k in ("id", "node", "priority", "req", "req_present"):
            assert np.array_equal(got[k], left[k]), f"{where}: surviving table, {k}"
        assert ctx.nominated_ids() == len(scn["nominees"]), f"{where}: the id space does not move"
        cn = ctx.seq_nominated_read()
        assert cn["n"] == len(model["consumed"]) and list(zip(cn["id"].tolist(), cn["pod"].tolist(), cn["node"].tolist())) == model["consumed"], f"{where}: consumed rows"
    else:
        with pytest.raises(capi.BsError) as e:
            ctx.seq_nominated_read()
        assert e.value.status == STATE, f"{where}: bs_seq_nominated_read is the nominated forms'"
    return r, model, (nodes, groups, wait)


# ---- the grid -------------------------------------------------------------------------------------------------------------------------------------
GRID_ROWS = [(ni, s) for ni, n in enumerate(sms.GRID_N) for s in sms.starts(n)]


@pytest.mark.parametrize("ni,start", GRID_ROWS, ids=[f"N{sms.GRID_N[ni]}-s{s}" for ni, s in GRID_ROWS])
def test_the_pass_equals_the_model_over_the_grid(ni, start):
    """one N and one cursor under every K of the grid: K = 1, 2, 64, 0 (all), N and N + 1"""
    cases = [c for c in sms.GRID_P if c[2] == ni and c[3] == start]
    assert [c[4] for c in cases] == sms.sizes(sms.GRID_N[ni])
    for j, case in enumerate(cases):
        with _open(case) as ctx:
            _check(ctx, case, flat=bool((ni + j) & 1))


@pytest.mark.parametrize("ni", range(len(sms.GRID_N)), ids=[f"N{n}" for n in sms.GRID_N])
def test_the_nominated_pass_equals_the_model_over_the_grid(ni):
    """rule SP underneath: every cursor and every K of the grid once per N, with rows in the candidate test and own rows consumed"""
    cases = [c for c in sms.GRID_SP if c[2] == ni]
    assert {c[3] for c in cases} == set(sms.starts(sms.GRID_N[ni])) and {c[4] for c in cases} == set(sms.sizes(sms.GRID_N[ni]))
    for j, case in enumerate(cases):
        with _open(case) as ctx:
            _check(ctx, case, flat=bool((ni + j) & 1))


@pytest.mark.parametrize("case", sms.KNOWN_CASES, ids=[f"K{c[3]}" for c in sms.KNOWN_CASES])
def test_k_around_a_candidate_set_of_known_size(case):
    """|C| = 12 for every pod: K = 11 stops on the twelfth member, K = 12 is all of C (V = N), K = 13 more than there is"""
    with _open(case) as ctx:
        r, model, _ = _check(ctx, case)
        assert model["n_fit"] == [min(case[3], sms.KNOWN_C)] * 10
        assert all(v == 200 for v in model["visited"]) == (case[3] >= sms.KNOWN_C)


@pytest.mark.parametrize("case", sms.FAR_CASES, ids=[f"K{c[3]}" for c in sms.FAR_CASES])
def test_a_walk_of_three_rounds_stops_in_a_later_round_and_in_the_revisited_lanes(case):
    """1025 nodes, six candidates: the member that ends the walk sits in round 1 (its predecessor in round 0), in round 2, and — K = 5 — in the
    lanes of the cursor's tile in front of the cursor, the walk's very last slot"""
    with _open(case) as ctx:
        r, model, _ = _check(ctx, case)
        assert model["visited"][0] == {1: 512, 2: 522, 4: 1016, 5: 1019}[case[3]] and model["hazards"]["d"] >= 1


# ---- the lane counts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sms.LANE_CASES, ids=[f"{c[1]}-S{c[2]}" for c in sms.LANE_CASES])
def test_every_lane_count_that_takes_another_path(case):
    """0, 1 and 4 scalar lanes keep everything in registers; 5, 9 and 12 take the lean form (the winner's lanes fetched behind the decision, the
    pod's scalar requests from the staged window, under rule SP one walk of a row chain per lane asked for)"""
    assert len(sms.scene(case)["names"]) == case[2]
    with _open(case) as ctx:
        r, model, _ = _check(ctx, case, flat=bool(case[2] & 1))
        assert sum(1 for a in model["assumed"] if a >= 0) >= 10 and model["hazards"]["a"] >= 1


# ---- F1 on twin contexts --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sms.F1_CASES, ids=["-".join(str(x) for x in c[:5]) for c in sms.F1_CASES])
def test_f1_all_nodes_from_cursor_zero_equal_the_parent_form_on_a_twin(case):
    key, sample, w, _ = sms.split(case)
    scn = sms.scene(case)
    table = scn["nominees"] is not None
    with _open(case) as a, _open(case) as b:
        ra = a.seq_run_scored_nominated(w, scn["priority"], scn["own_id"]) if table else a.seq_run_scored(w)
        rb = _run(b, case)
        for k in OUTPUTS:
            assert np.array_equal(ra[k], rb[k]), k
        for k in ("n_released", "node_picks", "node_scans"):
            assert ra[k] == rb[k], k
        assert (rb["pod_node"] >= 0).sum() > 0
        _same_state(_state(a, table), _state(b, table), "twin")
        assert_groups_equal(b.read_groups(), a.read_groups(), soa, "twin")
        assert np.array_equal(a.seq_waiting_read(), b.seq_waiting_read()) and a.find_max_pg() == b.find_max_pg()
        sa, sb = a.seq_score_read(), b.seq_score_read()
        assert np.array_equal(sa["total"], sb["total"]) and np.array_equal(sa["n_fit"], sb["n_fit"]) and sa["total"].any()
        if table:
            ca, cb = a.seq_nominated_read(), b.seq_nominated_read()
            assert ca["n"] == cb["n"] and all(np.array_equal(ca[k], cb[k]) for k in ("id", "pod", "node"))
        c = b.seq_sample_read()
        n = sms.to_soa(key)[0].n
        reached = sb["n_fit"] > 0
        assert not c["start"].any() and c["next_start"] == 0 and np.all(c["visited"][reached] == n) and set(c["visited"].tolist()) <= {0, n}


# ---- F2 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("grid", "P", 5, 100, 1, (0, 0, 0)), ("grid", "P", 8, 500, 7, (0, 0, 0)), ("grid", "SP", 5, 100, 1, (0, 0, 0))],
                         ids=lambda c: "-".join(str(x) for x in c[:5]))
def test_f2_zero_weights_are_first_fit_from_a_rotating_start(case):
    with _open(case) as ctx:
        r, model, _ = _check(ctx, case)
        assert not any(model["total"]) and sum(1 for a in model["assumed"] if a >= 0) >= 5
        if case[4] == 1 and case[1] == "P":                      # K = 1: every placed pod sits on the node its walk began at, or behind it
            assert all(v <= sms.GRID_N[case[2]] for v in model["visited"]) and len(set(model["start"])) > 3


# ---- tiles the bounds exclude ----------------------------------------------------------------------------------------------------------------------
def test_an_excluded_tile_between_the_kth_member_and_the_next_and_one_that_holds_the_cursor():
    """394 nodes, every tile but 1 and 3 holds a candidate; the walk starts at 200 (inside excluded tile 3) and its fifth and sixth members are
    nodes 10 and 130, across excluded tile 1: neither C' nor V moves for the tiles that are never read"""
    case = sms.PRUNE_CASE
    with _open(case) as ctx:
        r, model, _ = _check(ctx, case)
        assert (model["start"][0], model["visited"][0], model["n_fit"][0]) == (200, 324, 5) and model["start"][1] == 130
        _wave0_reads_no_excluded_tile(r, model, [200, 130, 3, 330], 3)
    case = sms.PRUNE_CASE_1                                      # ... and from a cursor inside excluded tile 1
    with _open(case) as ctx:
        r, model, _ = _check(ctx, case)
        _wave0_reads_no_excluded_tile(r, model, [70, 3, 330, 140], 3)


def _wave0_reads_no_excluded_tile(r, model, starts, want):
    """bs_seq_out.pick_rounds is the tiles WAVE 0 read (the work counters are thread 0's).  With seven tiles every walk is one round and wave 0
    has the slot that begins at the cursor: it reads one tile per pod, none where the cursor's tile is an excluded one.  An exact count."""
    open_tiles = {k >> 6 for k in sms.PRUNE_OPEN}
    assert open_tiles == {0, 2, 4, 5, 6} and model["start"] == starts
    assert sum(int((s >> 6) in open_tiles) for s in starts) == want == r["pick_rounds"], "the cursor's tile holds no candidate: skipped, not read"


# ---- the Filter stage on the plain form ---------------------------------------------------------------------------------------------------------------
def test_filter_removes_the_node_that_would_have_been_the_kth_member():
    case = sms.FILTER_CASE
    with _open(case) as ctx:
        r, model, _ = _check(ctx, case)
        assert model["hazards"]["m"] >= 1 and not r["last_permitted"].any()


# ---- the cursor handed from pass to pass ----------------------------------------------------------------------------------------------------------------
def test_the_cursor_chains_across_two_passes_on_one_context(orc):
    case = sms.CHAIN_CASE
    key, sample, w, _ = sms.split(case)
    nodes0, fit, groups0, pods, _, _ = sms.to_soa(key)
    with _open(case) as ctx:
        r1, model, (nodes, groups, _) = _check(ctx, case)
        nxt = ctx.seq_sample_read()["next_start"]
        assert nxt == model["next_start"] and nxt not in (0, sample[1])
        # the second pass on the model: the array model from the state the first left, the cursor handed over
        ch = smsoa.SampledChoice((sample[0], nxt), w, pods.p, nodes.n)
        m2 = ssoa.seq_pass(orc, nodes, fit, groups, pods, model["pf_leader"][-1], ch)
        r2 = ctx.seq_run_scored_sampled(w, (sample[0], nxt))
        for k in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods"):
            assert np.array_equal(r2[k], m2[k]), f"the second pass: {k}"
        c2, s2 = ctx.seq_sample_read(), ctx.seq_score_read()
        assert np.array_equal(c2["start"], ch.start) and np.array_equal(c2["visited"], ch.visited) and c2["next_start"] == ch.next_start
        assert np.array_equal(s2["total"], ch.total) and np.array_equal(s2["n_fit"], ch.n_fit)
        req, pres = ctx.read_node_requests()
        assert np.array_equal(req, m2["nodes"].requested) and np.array_equal(pres, m2["nodes"].requested_present)
        assert_groups_equal(ctx.read_groups(), m2["groups"], soa, "the second pass")
        first = next(i for i in range(pods.p) if ch.n_fit[i] or ch.visited[i])
        assert c2["start"][first] == nxt and (m2["assumed"] >= 0).sum() > 0, "the second pass begins where the first ended, and places pods"


# ---- one real cycle behind the pass ------------------------------------------------------------------------------------------------------------------
def test_expire_release_park_and_bind_behind_the_pass(orc):
    case = ("grid", "P", 5, 64, 2, (1, 0, 1))                     # 129 nodes, four scalar lanes, gangs
    parts = sms.to_soa(sms.split(case)[0])
    pods, S, N, G = parts[3], parts[0].lanes - 4, parts[0].n, parts[2].g
    rng = np.random.default_rng(41)
    with _open(case) as ctx:
        r, model, (nodes, groups, wait) = _check(ctx, case)
        waiting_groups = sorted({int(pods.group[i]) for i in np.nonzero(wait >= 0)[0]})
        assert len(waiting_groups) >= 1 and (r["pod_node"] >= 0).sum() >= 2, "a gang that missed its quorum, and placed pods"
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
        w.release("release (an empty table)", [int(g) for g in r["released_group"]])
        pk = w.park("park")
        assert pk["n"] == int((wait >= 0).sum()) - exp["n_pods"] and np.all(ctx.seq_waiting_read() == -1)
        bound = three_valued(rng, N, 30, S)
        ctx.load_bound(bound)
        pl = np.nonzero(r["pod_node"] >= 0)[0]
        b = B(ctx, soa, bar.Table(bound, S, N), w.tab, N, G, pods=pods, pod_node=r["pod_node"].astype(np.int32), wait_node=st.wait_node, window=True)
        out = b.bind("bind the placed pods", (), pl, rng.integers(0, 3, pl.size).astype(np.int32), rng.integers(0, 3, pl.size).astype(np.int64))
        assert np.array_equal(out["node"], r["pod_node"][pl].astype(np.uint32)), "a placed pod brings the node the sampled pass chose"


# ---- the hand-derived answers on the device ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(KATS)), ids=[k["name"] for k in KATS])
def test_hand_answers_on_the_device(i):
    kat, case = KATS[i], ("kat", KATS[i]["form"], i)
    ex = kat["expect"]
    with _open(case) as ctx:
        r, model, (_, _, wait) = _check(ctx, case)
        s, c = ctx.seq_score_read(), ctx.seq_sample_read()
        assert np.where(r["pod_node"] >= 0, r["pod_node"], wait).tolist() == ex["assumed"], kat["why"]
        assert s["total"].tolist() == ex["total"] and s["n_fit"].tolist() == ex["n_fit"], kat["why"]
        assert c["start"].tolist() == ex["start"] and c["visited"].tolist() == ex["visited"] and c["next_start"] == ex["next_start"], kat["why"]
        if kat["form"] == "SP":
            assert ctx.nominated_read()["id"].tolist() == ex["rows_left"], kat["why"]


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_plain_form_and_nothing_changes():
    case = ("grid", "P", 5, 64, 2, (1, 0, 1))
    nodes, fit, groups, pods, _, _ = sms.to_soa(sms.split(case)[0])
    lib = capi.load_library()
    w, smp = (1, 0, 1), (2, 64)
    with _open(case) as ctx:
        before = _state(ctx, False)

        def refused(status, where, fn):
            with pytest.raises(capi.BsError) as e:
                fn()
            assert e.value.status == status, (where, str(e.value))
            _same_state(before, _state(ctx, False), where)

        # what bs_seq_run_scored refuses, with its codes
        refused(INVALID, "no PREFILTER", lambda: ctx.seq_run_scored_sampled(w, smp, stages=soa.STAGE_FILTER))
        refused(INVALID, "no stage at all", lambda: ctx.seq_run_scored_sampled(w, smp, stages=0))
        refused(INVALID, "deny without FILTER", lambda: ctx.seq_run_scored_sampled(w, smp, stages=PF | soa.BATCH_FILTER_DENY))
        refused(INVALID, "NULL score", lambda: ctx.seq_run_scored_sampled(None, smp))
        for j in range(3):
            big = [1, 1, 1]
            big[j] = capi.SCORE_WEIGHT_MAX + 1
            refused(INVALID, f"weight {j} of 65 537", lambda: ctx.seq_run_scored_sampled(big, smp))
            refused(INVALID, f"weight {j} of 65 537, flat", lambda: ctx.seq_run_scored_sampled(big, smp, flat=True))
        # ... then its own
        refused(INVALID, "NULL sample", lambda: ctx.seq_run_scored_sampled(w, None))
        refused(INVALID, "BS_BATCH_FILTER_DENY", lambda: ctx.seq_run_scored_sampled(w, smp, stages=DENY))
        refused(INVALID, "BS_BATCH_FILTER_DENY, flat", lambda: ctx.seq_run_scored_sampled(w, smp, stages=DENY, flat=True))
        refused(STATE, "bs_seq_sample_read before any pass", ctx.seq_sample_read)
        ctx.set_shard(0, 2)
        refused(STATE, "a sharded context", lambda: ctx.seq_run_scored_sampled(w, smp))
        ctx.set_shard(0, 1)
        ctx.reduce_external(True)
        refused(STATE, "an external-reduce context", lambda: ctx.seq_run_scored_sampled(w, smp))
        ctx.reduce_external(False)
        # every other pass clears the sampled read; a sampled pass answers all of its reads
        ctx.seq_run_scored(w)
        before = _state(ctx, False)
        refused(STATE, "bs_seq_sample_read after bs_seq_run_scored", ctx.seq_sample_read)
        ctx.seq_run_scored_sampled((capi.SCORE_WEIGHT_MAX,) * 3, (0xFFFFFFFF, 0xFFFFFFFF))        # the largest weights, K and start are fine
        before = _state(ctx, False)
        c0, s0 = ctx.seq_sample_read(), ctx.seq_score_read()
        assert int(c0["start"].max()) < nodes.n and int(c0["visited"].max()) == nodes.n, "K above N is all; the start is taken mod N"
        refused(INVALID, "bs_seq_sample_read with p too small", lambda: ctx.seq_sample_read(p=pods.p - 1))
        refused(INVALID, "bs_seq_sample_read with p too large", lambda: ctx.seq_sample_read(p=pods.p + 1))
        refused(STATE, "bs_seq_nominated_read after the plain sampled form", ctx.seq_nominated_read)
        only = np.zeros(pods.p, np.uint32)                                     # any pointer may be NULL
        ctx._chk(lib.bs_seq_sample_read(ctx._h, pods.p, None, capi._u32p(only), None), "bs_seq_sample_read")
        assert only.tolist() == c0["visited"].tolist()
        nxt = capi.C.c_uint32(77)
        ctx._chk(lib.bs_seq_sample_read(ctx._h, pods.p, None, None, capi.C.byref(nxt)), "bs_seq_sample_read")
        assert nxt.value == c0["next_start"]
        ctx._chk(lib.bs_seq_sample_read(ctx._h, pods.p, None, None, None), "bs_seq_sample_read")
        refused(INVALID, "a NULL sample after a good pass", lambda: ctx.seq_run_scored_sampled(w, None))
        c1 = ctx.seq_sample_read()
        assert all(np.array_equal(c0[k], c1[k]) for k in ("start", "visited")) and c0["next_start"] == c1["next_start"], "a refused pass leaves the last one readable"
        assert np.array_equal(s0["n_fit"], ctx.seq_score_read()["n_fit"])
        ctx.seq_run(PF)
        before = _state(ctx, False)
        refused(STATE, "bs_seq_sample_read after a plain bs_seq_run", ctx.seq_sample_read)
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:                     # what bs_seq_run refuses, with its code
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_scored_sampled(w, smp)
        assert e.value.status == STATE


def test_every_refusal_of_the_nominated_form_and_nothing_changes():
    case = ("grid", "SP", 5, 64, 2, (1, 0, 1))
    scn = sms.scene(case)
    nodes, fit, groups, pods, _, tab = sms.to_soa(sms.split(case)[0])
    prio, own, P, w, smp = scn["priority"], scn["own_id"], len(scn["priority"]), (1, 0, 1), (2, 64)
    with _open(case) as ctx:
        before = _state(ctx, True)

        def refused(status, where, *a, **kw):
            with pytest.raises(capi.BsError) as e:
                ctx.seq_run_scored_nominated_sampled(*a, **kw)
            assert e.value.status == status, (where, str(e.value))
            _same_state(before, _state(ctx, True), where)
            for read in (ctx.seq_nominated_read, ctx.seq_score_read, ctx.seq_sample_read):   # no pass has run: every read refuses
                with pytest.raises(capi.BsError) as e2:
                    read()
                assert e2.value.status == STATE, where

        # what bs_seq_run_scored_nominated refuses, in its order
        refused(INVALID, "no PREFILTER", w, smp, prio, own, stages=soa.STAGE_FILTER)
        refused(INVALID, "FILTER", w, smp, prio, own, stages=FILTER)
        refused(INVALID, "FILTER + deny", w, smp, prio, own, stages=DENY)
        refused(INVALID, "deny without FILTER", w, smp, prio, own, stages=PF | soa.BATCH_FILTER_DENY)
        refused(INVALID, "p too small", w, smp, prio, own, p=P - 1)
        refused(INVALID, "p too large", w, smp, prio, own, p=P + 1)
        refused(INVALID, "NULL priority", w, smp, None, own)
        bad = own.copy()
        bad[np.nonzero(own == capi.NOM_NONE)[0][0]] = len(scn["nominees"])
        refused(INVALID, "unknown own id", w, smp, prio, bad)
        refused(INVALID, "NULL score", None, smp, prio, own)
        refused(INVALID, "a weight of 65 537", (1, capi.SCORE_WEIGHT_MAX + 1, 1), smp, prio, own)
        refused(INVALID, "a weight of 65 537, flat", (1, capi.SCORE_WEIGHT_MAX + 1, 1), smp, prio, own, flat=True)
        # ... then its own
        refused(INVALID, "NULL sample", w, None, prio, own)
        for where, on, off in (("a sharded context", lambda: ctx.set_shard(0, 2), lambda: ctx.set_shard(0, 1)),
                               ("an external-reduce context", lambda: ctx.reduce_external(True), lambda: ctx.reduce_external(False))):
            on()                                                                 # (the table's own reads are single-rank only: compare once it is off again)
            with pytest.raises(capi.BsError) as e:
                ctx.seq_run_scored_nominated_sampled(w, smp, prio, own)
            assert e.value.status == STATE, where
            off()
            _same_state(before, _state(ctx, True), where)
        # a good pass answers all three reads; the parent form behind it clears the sampled one
        ctx.seq_run_scored_nominated_sampled(w, smp, prio, own)
        assert ctx.seq_sample_read()["visited"].any() and ctx.seq_nominated_read()["n"] > 0 and ctx.seq_score_read()["n_fit"].any()
        keep = np.full(P, capi.NOM_NONE, np.uint32)
        ctx.seq_run_scored_nominated(w, prio, keep)
        with pytest.raises(capi.BsError) as e:
            ctx.seq_sample_read()
        assert e.value.status == STATE
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:                       # no table at all
        req0, _ = ctx.read_node_requests()
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_scored_nominated_sampled(w, smp, prio, None)
        assert e.value.status == STATE and np.array_equal(req0, ctx.read_node_requests()[0])


# ---- the flat twins ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("grid", "P", 5, 64, 2, (3, 2, 1)), ("grid", "SP", 5, 64, 2, (3, 2, 1))], ids=["plain", "nominated"])
def test_the_flat_twins_equal_the_struct_forms(case):
    table = case[1] == "SP"
    with _open(case) as a, _open(case) as b:
        ra, rb = _run(a, case, flat=False), _run(b, case, flat=True)
        for k in OUTPUTS + ("n_released", "node_picks", "node_scans"):
            assert np.array_equal(ra[k], rb[k]), k
        _same_state(_state(a, table), _state(b, table), "flat twin")
        ca, cb, sa, sb = a.seq_sample_read(), b.seq_sample_read(), a.seq_score_read(), b.seq_score_read()
        assert all(np.array_equal(ca[k], cb[k]) for k in ("start", "visited")) and ca["next_start"] == cb["next_start"] and ca["visited"].any()
        assert np.array_equal(sa["total"], sb["total"]) and np.array_equal(sa["n_fit"], sb["n_fit"])
