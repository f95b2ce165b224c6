"""GPU tests of bs_seq_run_scored (include/bsched.h, rule P / D7; csrc/bs_seq.hpp, seq_pick_scored and k_seq_scored<TS>): the sequential pass
with the scored node choice against the object-level model tests/seq_scored_ref.py, bit for bit — every output, the totals and candidate
counts, the node requests and group state the pass leaves; zero weights against bs_seq_run on a twin context; the geometry of the kernel's
tile walk by construction; identical nodes; lanes outside the rule's domain; the Filter stage with and without its TTL writes; one real
cycle behind the pass; every refusal; and a plain pass behind a scored one.  Scenes are small (the parity set: 1 to 513 nodes, at most 200
pods) except the one that needs two tile walks (32 838 nodes, six pods, all tiles but three pruned); models are computed once per scene.
tests/test_seq_scored_cpu.py asserts that this scene set meets every hazard letter of the model."""
import functools
import importlib

import numpy as np
import pytest

import bound_apply_ref as bar
import bound_bind_ref as bbr
import seq_expire_ref as sx
import seq_scored_ref as ssr
import seq_scored_scenes as sss
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


@functools.lru_cache(maxsize=None)
def _scene(key):
    """(scene, its SoA): computed once, never changed"""
    kind = key[0]
    if kind == "parity":
        sc = sss.parity_scene(*key[1:])
    elif kind == "filter":
        sc = sss.filter_scene(key[1])
    elif kind == "kat":
        sc = sss.kat_scene(sss.load_kats()["scenes"][key[1]])
    else:
        sc = getattr(sss, kind)()
    return sc, sss.to_soa(sc)


@functools.lru_cache(maxsize=None)
def _model(key, weights, stages=PF):
    sc = _scene(key)[0]
    return ssr.replay(sc, weights, run_filter=bool(stages & soa.STAGE_FILTER), filter_deny=bool(stages & soa.BATCH_FILTER_DENY), scalar_names=sc["names"])


def _open(key):
    nodes, fit, groups, pods, _ = _scene(key)[1]
    return load_ctx(bsa, nodes, fit, groups, pods)


def _state(ctx):
    req, pres = ctx.read_node_requests()
    g = ctx.read_groups()
    return dict(req=req, pres=pres, matched=g.matched.copy(), flags=g.flags.copy(), sc=g.status_scheduled.copy(), cls=g.cls.copy(), mr=g.min_resources.copy(),
                occ=g.occupied_by.copy())


def _same_state(a, b, where):
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{where}: {k} changed"


def _check(ctx, key, weights, where, stages=PF, flat=False):
    """one bs_seq_run_scored on ctx against the model of scene `key`"""
    (sc, parts), model = _scene(key), _model(key, weights, stages)
    r = ctx.seq_run_scored(weights, stages=stages, flat=flat)
    for k in OUTPUTS:
        assert r[k].tolist() == list(model[k]), f"{where}: {k}"
    s = ctx.seq_score_read()
    assert s["total"].tolist() == model["total"], f"{where}: total"
    assert s["n_fit"].tolist() == model["n_fit"], f"{where}: n_fit"
    nodes, groups, wait = ssr.end_state_soa(model, sc, soa, dict(parts[4]))
    req, pres = ctx.read_node_requests()
    assert np.array_equal(req, nodes.requested), f"{where}: node requests after the pass"
    assert np.array_equal(pres, nodes.requested_present), f"{where}: node request keys"
    assert_groups_equal(ctx.read_groups(), groups, soa, where)
    assert np.array_equal(ctx.seq_waiting_read(), wait), f"{where}: the pods still waiting at Permit"
    assumed = np.where(r["pod_node"] >= 0, r["pod_node"], wait)
    assert assumed.tolist() == model["assumed"], f"{where}: the node every pod was assumed on"
    return r, model, (nodes, groups, wait)


# ---- P2: zero weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,stages", [(("parity",) + sss.PARITY[4], PF), (("parity",) + sss.PARITY[5], PF), (("parity",) + sss.PARITY[7], PF), (("parity",) + sss.PARITY_MAX[0], PF), (("parity",) + sss.PARITY_MAX[3], DENY),
                                        (("parity",) + sss.PARITY[9], FILTER), (("filter", 9105), DENY)], ids=lambda v: str(v))
def test_zero_weights_equal_bs_seq_run_on_a_twin(key, stages):
    model = _model(key, (0, 0, 0), stages)
    with _open(key) as a, _open(key) as b:
        ra, rb = a.seq_run(stages), b.seq_run_scored((0, 0, 0), stages=stages)
        for k in OUTPUTS:
            assert np.array_equal(ra[k], rb[k]), k
        for k in ("n_released", "node_picks", "node_scans"):
            assert ra[k] == rb[k], k
        assert (rb["pod_node"] >= 0).sum() > 0
        _same_state(_state(a), _state(b), "twin")
        assert_groups_equal(b.read_groups(), a.read_groups(), soa, "twin")
        assert np.array_equal(a.seq_waiting_read(), b.seq_waiting_read())
        s = b.seq_score_read()
        assert s["n_fit"].tolist() == model["n_fit"] and not s["total"].any()
        assert a.find_max_pg() == b.find_max_pg()


# ---- model parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(sss.PARITY)), ids=[f"{s}-N{n}-S{S}-{'gangs' if g else 'single'}" for s, n, S, g in sss.PARITY])
def test_the_pass_equals_the_model(i):
    key, weights = ("parity",) + sss.PARITY[i], sss.WEIGHTS[i % len(sss.WEIGHTS)]
    with _open(key) as ctx:
        _check(ctx, key, weights, f"{key} {weights}", flat=bool(i & 1))


@pytest.mark.parametrize("i", range(len(sss.PARITY_MAX)), ids=[f"{s}-N{n}-S{S}-{'gangs' if g else 'single'}" for s, n, S, g in sss.PARITY_MAX])
def test_the_pass_equals_the_model_at_the_maximum_lane_count(i):
    """12 scalar lanes, and 5 and 9: above 4 the kernel is built lean — the search keeps its key only and fetches the winner's lanes behind
    the decision, the pod's scalar requests come from the staged window, PreFilter scans without table summaries (csrc/bs_seq.hpp)"""
    key, weights = ("parity",) + sss.PARITY_MAX[i], sss.WEIGHTS[(3 + i) % len(sss.WEIGHTS)]
    with _open(key) as ctx:
        _check(ctx, key, weights, f"{key} {weights}")


@pytest.mark.parametrize("weights", sss.WEIGHTS, ids=str)
@pytest.mark.parametrize("n", [65, 8 * 64 + 1])
def test_every_weight_triple_around_a_tile_border(n, weights):
    key = ("parity", 9140 + n, n, 1, True)
    with _open(key) as ctx:
        _check(ctx, key, weights, f"N {n} {weights}")


# ---- the hand-derived scenes on the device ---------------------------------------------------------------------------------------------------------
def test_hand_derived_scenes_on_the_device():
    for k, kat in enumerate(sss.load_kats()["scenes"]):
        for wtext, nodes in kat["expect"].items():
            w = tuple(int(x) for x in wtext.split(","))
            with _open(("kat", k)) as ctx:
                r, _, _ = _check(ctx, ("kat", k), w, f"{kat['name']} {wtext}")
                assert r["pod_node"].tolist() == nodes, kat["why"]


# ---- geometry by construction ------------------------------------------------------------------------------------------------------------------------
def test_two_tile_walks_and_the_tie_between_them():
    """candidates only on the last lane of the first walk's last tile, lane 0 of the second walk's first tile and the last valid node"""
    key, n = ("geometry_walks",), sss.WALK + 70
    with _open(key) as ctx:
        r, model, _ = _check(ctx, key, (1, 0, 1), "walks (1,0,1)")
        assert r["pod_node"].tolist() == [n - 1, sss.WALK - 1, sss.WALK, n - 1, sss.WALK - 1, sss.WALK], "the larger node first, then the tie across the walks to the lower index"
        assert model["n_fit"] == [3] * 6
    with _open(key) as ctx:
        r, _, _ = _check(ctx, key, (0, 1, 0), "walks (0,1,0)")
        assert r["pod_node"].tolist() == [sss.WALK - 1] * 4 + [sss.WALK] * 2


def test_a_winner_in_wave_one_a_second_tile_of_one_lane_and_a_tie_inside_a_tile():
    key = ("geometry_waves",)
    with _open(key) as ctx:
        r, _, _ = _check(ctx, key, (1, 0, 1), "waves (1,0,1)")
        assert r["pod_node"].tolist()[:4] == [65 * 64 + 5, 66 * 64 + 1, 66 * 64 + 9, 64 * 64 + 5]
    with _open(key) as ctx:
        _check(ctx, key, (0, 1, 0), "waves (0,1,0)")


# ---- identical nodes; lanes out of domain ------------------------------------------------------------------------------------------------------------
def test_identical_nodes_spread_and_pack():
    with _open(("identical",)) as ctx:
        r, _, _ = _check(ctx, ("identical",), (1, 0, 1), "spread")
        assert r["pod_node"].tolist() == [i % 8 for i in range(20)]
    with _open(("identical",)) as ctx:
        r, _, _ = _check(ctx, ("identical",), (0, 1, 0), "pack")
        assert r["pod_node"].tolist() == [i // 8 for i in range(20)]


@pytest.mark.parametrize("weights", [(1, 0, 1), (0, 1, 0), (3, 2, 1)], ids=str)
def test_lanes_out_of_domain_score_zero_and_stay_candidates(weights):
    with _open(("out_of_domain",)) as ctx:
        r, model, _ = _check(ctx, ("out_of_domain",), weights, f"out of domain {weights}")
        assert model["hazards"]["d"] == 18 and len(set(model["assumed"])) >= 4


# ---- the Filter stage ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [FILTER, DENY], ids=["filter", "filter+deny"])
@pytest.mark.parametrize("seed", [9105, 9109])
def test_filter_narrows_the_candidates(seed, stages):
    key = ("filter", seed)
    with _open(key) as ctx:
        r, model, _ = _check(ctx, key, (1, 0, 1), f"seed {seed} stages {stages}", stages=stages)
        assert model["hazards"]["i"] >= 1, "Filter removed the node that would have won"
        if stages == DENY:
            assert sum(model["last_permitted"]) > 0 and sum(model["denied"]) > 0
            assert r["last_permitted"].tolist() == model["last_permitted"]


# ---- one real cycle behind the scored pass ---------------------------------------------------------------------------------------------------------
def test_expire_release_park_and_bind_behind_the_pass(orc):
    key, weights = ("parity",) + sss.PARITY[4], (1, 0, 1)          # 130 nodes, one scalar lane, gangs
    (sc, parts) = _scene(key)
    pods, S, N, G = parts[3], parts[0].lanes - 4, parts[0].n, parts[2].g
    rng = np.random.default_rng(31)
    with _open(key) as ctx:
        r, model, (nodes, groups, wait) = _check(ctx, key, weights, "the pass")
        waiting_groups = sorted({int(pods.group[i]) for i in np.nonzero(wait >= 0)[0]})
        assert len(waiting_groups) >= 2 and (r["pod_node"] >= 0).sum() >= 2, "gangs that missed their quorum, and placed pods"
        st = sx.State(nodes.requested, nodes.requested_present, groups.matched, groups.flags, wait)
        # the Permit timeout of one gang that missed its quorum
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
        assert np.array_equal(out["node"], r["pod_node"][pl].astype(np.uint32)), "a placed pod brings the node the scored pass chose"


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_and_nothing_changes():
    key = ("parity",) + sss.PARITY[4]
    nodes, fit, groups, pods, _ = _scene(key)[1]
    lib = capi.load_library()
    with _open(key) as ctx:
        before = _state(ctx)

        def refused(status, where, fn):
            with pytest.raises(capi.BsError) as e:
                fn()
            assert e.value.status == status, (where, str(e.value))
            _same_state(before, _state(ctx), where)

        def raw(score, stages=PF):
            o = capi.SeqOut()
            ctx._chk(lib.bs_seq_run_scored(ctx._h, stages, score, capi.C.byref(o)), "bs_seq_run_scored")

        refused(INVALID, "NULL score", lambda: raw(None))
        for j in range(3):
            w = [1, 1, 1]
            w[j] = capi.SCORE_WEIGHT_MAX + 1
            refused(INVALID, f"weight {j} of 65 537", lambda: ctx.seq_run_scored(w))
            refused(INVALID, f"weight {j} of 65 537, flat", lambda: ctx.seq_run_scored(w, flat=True))
        refused(INVALID, "no PREFILTER", lambda: ctx.seq_run_scored((1, 0, 1), stages=soa.STAGE_FILTER))
        refused(INVALID, "deny without FILTER", lambda: ctx.seq_run_scored((1, 0, 1), stages=PF | soa.BATCH_FILTER_DENY))
        refused(INVALID, "no stage at all", lambda: ctx.seq_run_scored((1, 0, 1), stages=0))
        refused(STATE, "bs_seq_score_read before any pass", ctx.seq_score_read)
        ctx.set_shard(0, 2)
        refused(STATE, "a sharded context", lambda: ctx.seq_run_scored((1, 0, 1)))
        ctx.set_shard(0, 1)
        ctx.reduce_external(True)
        refused(STATE, "an external-reduce context", lambda: ctx.seq_run_scored((1, 0, 1)))
        ctx.reduce_external(False)
        ctx.seq_run(PF)                                                        # a plain pass: not the scored call's
        before = _state(ctx)
        refused(STATE, "bs_seq_score_read after a plain bs_seq_run", ctx.seq_score_read)
        ctx.seq_run_scored((capi.SCORE_WEIGHT_MAX,) * 3)                       # the largest weights are fine
        before = _state(ctx)
        assert int(ctx.seq_score_read()["total"].max()) < 1 << 32
        refused(INVALID, "bs_seq_score_read with p too small", lambda: ctx.seq_score_read(p=pods.p - 1))
        refused(INVALID, "bs_seq_score_read with p too large", lambda: ctx.seq_score_read(p=pods.p + 1))
        refused(STATE, "bs_seq_nominated_read after a scored pass", ctx.seq_nominated_read)
        only = np.zeros(pods.p, np.uint32)                                     # either pointer may be NULL
        ctx._chk(lib.bs_seq_score_read(ctx._h, pods.p, None, capi._u32p(only)), "bs_seq_score_read")
        assert only.tolist() == ctx.seq_score_read()["n_fit"].tolist()
        ctx._chk(lib.bs_seq_score_read(ctx._h, pods.p, None, None), "bs_seq_score_read")
        refused(INVALID, "a weight above the maximum after a good pass", lambda: ctx.seq_run_scored((0, 0, 65537)))
        assert ctx.seq_score_read()["n_fit"].tolist() == only.tolist(), "a refused pass leaves the last one readable"
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:                     # what bs_seq_run refuses, with its code
        with pytest.raises(capi.BsError) as e:
            ctx.seq_run_scored((1, 0, 1))
        assert e.value.status == STATE
    o = capi.SeqOut()
    assert lib.bs_seq_run_scored(None, 1, None, capi.C.byref(o)) == INVALID and lib.bs_seq_score_read(None, 0, None, None) == INVALID


# ---- a plain pass behind a scored one ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [4, 6])
def test_a_plain_pass_behind_a_scored_one_equals_the_oracle_from_that_state(i, orc):
    key, weights = ("parity",) + sss.PARITY[i], (1, 0, 1)
    fit, pods = _scene(key)[1][1], _scene(key)[1][3]
    with _open(key) as ctx:
        _, model, (nodes, groups, _) = _check(ctx, key, weights, "the scored pass")
        s2 = orc.seq_replay(nodes, fit, groups, pods, PF, leader=model["pf_leader"][-1])
        r2 = ctx.seq_run(PF)
        for k in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods"):
            assert np.array_equal(r2[k], s2[k]), f"the plain pass: {k}"
        req, pres = ctx.read_node_requests()
        assert np.array_equal(req, s2["nodes"].requested) and np.array_equal(pres, s2["nodes"].requested_present)
        assert_groups_equal(ctx.read_groups(), s2["groups"], soa, "the plain pass")
        assert (r2["pod_node"] >= 0).sum() + (ctx.seq_waiting_read() >= 0).sum() > 0, "the second pass placed pods"
        with pytest.raises(capi.BsError) as e:
            ctx.seq_score_read()
        assert e.value.status == STATE
