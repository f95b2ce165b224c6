"""CPU tests of PDB-aware preemption's restatements (tests/preempt_pdb_ref.py) and of the host helper batch-scheduler_amd/pdb.py: the
hand known answers (tests/golden/preempt_pdb_hand_kats.json) against both restatements, the restatements against each other on seeded
random scenes, both against preempt_ref / preempt_commit_ref with every bit clear, the conditions that keep the random scenes from
passing vacuously, and the matching rules."""
import importlib

import numpy as np
import pytest

import preempt_commit_ref as pc
import preempt_pdb_ref as pp
import preempt_ref as pr

bsa = importlib.import_module("batch-scheduler_amd")
pdb = importlib.import_module("batch-scheduler_amd.pdb")


def _args(s):
    return s["nodes"], s["fit"], s["pods"], s["bound"], s["S"], s["pod_index"], s["priority"], s["protected"]


def _commit_both(s, cap, bits, apply=False, assume=False):
    obj = pp.commit_pdb_obj(*_args(s), cap, bits, apply, assume)
    nump = pp.commit_pdb_np(pp.PdbPrep(s["nodes"], s["bound"], s["S"], bits), s["fit"], s["pods"], s["bound"], s["pod_index"], s["priority"],
                            s["protected"], cap, apply, assume)
    return obj, nump


def _run_both(s, cap, bits):
    obj = pp.preempt_pdb_obj(*_args(s), cap, bits)
    nump = pp.preempt_pdb_np(pp.PdbPrep(s["nodes"], s["bound"], s["S"], bits), s["fit"], s["pods"], s["pod_index"], s["priority"], s["protected"], cap)
    return obj, nump


def _same(a, b, where, fields=pp.FIELDS):
    for f in fields:
        assert np.array_equal(a[f], b[f]), f"{where}: {f} {a[f]} vs {b[f]}"


def _same_state(a, b, where):
    for f in ("req", "pres", "bound_id", "bound_node"):
        assert np.array_equal(a[f], b[f]), f"{where}: {f}"


@pytest.mark.parametrize("sc", pp.pdb_kats(), ids=lambda s: s["name"])
def test_hand_known_answers(sc):
    s = pp.kat_pdb_scene(sc)
    for name, got in zip(("object", "numpy"), _commit_both(s, s["cap"], s["violating"])):
        pp.check_pdb_kat(got, sc, f"{name} {sc['name']}")
    if len(sc["expect"]) == 1:                              # slot 0 of a plan is bs_preempt_run's answer
        for name, got in zip(("object", "numpy"), _run_both(s, s["cap"], s["violating"])):
            pp.check_pdb_kat(dict(res=got), sc, f"run {name} {sc['name']}")


def test_every_known_answer_needs_its_bits():
    """an implementation that accepts the bits and ignores them fails every scene but the ones that pin a count of 0 on an unchanged pick"""
    differ = 0
    for sc in pp.pdb_kats():
        s = pp.kat_pdb_scene(sc)
        with_bits = pp.commit_pdb_np(pp.PdbPrep(s["nodes"], s["bound"], s["S"], s["violating"]), s["fit"], s["pods"], s["bound"], s["pod_index"],
                                     s["priority"], s["protected"], s["cap"])["res"]
        none = pp.commit_pdb_np(pp.PdbPrep(s["nodes"], s["bound"], s["S"], None), s["fit"], s["pods"], s["bound"], s["pod_index"], s["priority"],
                                s["protected"], s["cap"])["res"]
        differ += any(not np.array_equal(with_bits[f], none[f]) for f in pp.FIELDS)
    assert differ >= 8, differ


# (S, nodes, per node, preemptors, groups, bit share)
RANDOM = [(0, 12, (5, 15), 30, 0, 0.6), (1, 40, (0, 12), 20, 6, 0.5), (4, 30, (2, 20), 24, 6, 0.5), (12, 25, (0, 10), 16, 0, 0.5)]


def _scenes(case, count=8):
    S, n, per, q, groups, share = case
    for seed in range(count):
        sc, bits = pp.pdb_scene(7000 + 31 * seed + S, n, per, S, q, groups, share)
        yield seed, sc, bits


@pytest.mark.parametrize("case", RANDOM, ids=str)
def test_restatements_agree_and_the_bits_matter(case):
    seen, changed, total = set(), 0, 0
    for seed, sc, bits in _scenes(case):
        S = sc["S"]
        obj, nump = _run_both(sc, 5, bits)
        _same(obj, nump, f"run seed {seed}")
        plain = pr.preempt_np(pr.Prep(sc["nodes"], sc["bound"], S), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], 5)
        clear_obj, clear_np = _run_both(sc, 5, np.zeros(sc["bound"].b, np.uint8))
        _same(clear_obj, plain, f"clear bits, object, seed {seed}", pr_fields)
        _same(clear_np, plain, f"clear bits, numpy, seed {seed}", pr_fields)
        assert not clear_np["n_pdb_violations"].any() and not clear_obj["n_pdb_violations"].any()
        e = pp.effects(sc, nump, plain, bits)
        seen |= e
        changed += "changed" in e
        total += 1
        for apply, assume in ((False, False), (True, False), (True, True)):
            cobj, cnp = _commit_both(sc, 5, bits, apply, assume)
            _same(cobj["res"], cnp["res"], f"commit seed {seed} apply={apply} assume={assume}")
            _same_state(cobj, cnp, f"commit state seed {seed} apply={apply} assume={assume}")
            z = np.zeros(sc["bound"].b, np.uint8)
            cz = pp.commit_pdb_np(pp.PdbPrep(sc["nodes"], sc["bound"], S, z), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"],
                                  sc["protected"], 5, apply, assume)
            cp = pc.commit_np(pc.CommitPrep(sc["nodes"], sc["bound"], S), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"],
                              sc["protected"], 5, apply, assume)
            _same(cz["res"], cp["res"], f"commit clear bits seed {seed}", pr_fields)
            _same_state(cz, cp, f"commit clear bits state seed {seed}")
    assert 4 * changed >= total, f"the bits changed the answer in {changed} of {total} scenes"
    missing = [x for x in pp.EFFECTS if x not in seen]
    assert not missing, f"effects never seen over the scene set: {missing}"


pr_fields = ("node", "n_candidates", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start")


# ---- the host helper
def _pod(ns="a", **labels):
    return {"namespace": ns, "labels": labels or None}


def _pdb(ns="a", allowed=0, selector=None):
    return {"namespace": ns, "selector": selector, "disruptions_allowed": allowed}


def test_matching_rules():
    web = {"matchLabels": {"app": "web"}}
    pods = [_pod(app="web"), _pod(app="db"), _pod("b", app="web"), _pod(), _pod(app="web", tier="x")]
    assert pdb.violating_bits([_pdb(selector=web)], pods).tolist() == [1, 0, 0, 0, 1]             # M1, M2
    assert pdb.violating_bits([_pdb(selector=web, allowed=1)], pods).tolist() == [0] * 5           # M5
    assert pdb.violating_bits([_pdb(selector=web, allowed=-1)], pods).tolist() == [1, 0, 0, 0, 1]
    assert pdb.violating_bits([_pdb(selector=web, allowed=3), _pdb(selector=web, allowed=0)], pods).tolist() == [1, 0, 0, 0, 1]   # any PDB
    assert pdb.violating_bits([_pdb(selector=None)], pods).tolist() == [0] * 5                     # M4: nil
    assert pdb.violating_bits([_pdb(selector={})], pods).tolist() == [0] * 5                       # M4: empty
    assert pdb.violating_bits([_pdb(selector={"matchLabels": {}, "matchExpressions": []})], pods).tolist() == [0] * 5
    assert pdb.violating_bits([], pods).tolist() == [0] * 5


def test_match_expressions():
    pods = [_pod(app="web"), _pod(app="db"), _pod(tier="x"), _pod()]

    def bits(*exprs):
        return pdb.violating_bits([_pdb(selector={"matchExpressions": list(exprs)})], pods).tolist()

    assert bits({"key": "app", "operator": "In", "values": ["web", "api"]}) == [1, 0, 0, 0]
    assert bits({"key": "app", "operator": "NotIn", "values": ["web"]}) == [0, 1, 1, 0]            # a pod without the key matches NotIn
    assert bits({"key": "app", "operator": "Exists"}) == [1, 1, 0, 0]
    assert bits({"key": "app", "operator": "DoesNotExist"}) == [0, 0, 1, 0]                          # the unlabelled pod: M2
    assert bits({"key": "app", "operator": "Exists"}, {"key": "app", "operator": "NotIn", "values": ["db"]}) == [1, 0, 0, 0]
    both = {"matchLabels": {"app": "web"}, "matchExpressions": [{"key": "tier", "operator": "DoesNotExist"}]}
    assert pdb.violating_bits([_pdb(selector=both)], pods + [_pod(app="web", tier="x")]).tolist() == [1, 0, 0, 0, 0]


@pytest.mark.parametrize("selector", [
    {"matchExpressions": [{"key": "app", "operator": "Gt", "values": ["1"]}]},       # not a label-selector operator
    {"matchExpressions": [{"key": "app", "operator": "In", "values": []}]},
    {"matchExpressions": [{"key": "app", "operator": "Exists", "values": ["x"]}]},
    {"matchExpressions": [{"key": "bad key", "operator": "Exists"}]},
    {"matchLabels": {"app": "not a value!"}},
    {"matchLabels": {"": "x"}},
])
def test_unparsable_selector_is_skipped(selector):
    pods = [_pod(app="web")]
    with pytest.raises(ValueError):
        pdb.parse_selector(selector)
    good = _pdb(selector={"matchLabels": {"app": "web"}})
    assert pdb.violating_bits([_pdb(selector=selector)], pods).tolist() == [0]                    # M3
    assert pdb.violating_bits([_pdb(selector=selector), good], pods).tolist() == [1]


def test_abi_lists_the_new_entry_points():
    capi = importlib.import_module("batch-scheduler_amd.capi")
    assert "bs_bound_pdb_set" in capi.ABI_SYMBOLS and "bs_preempt_pdb_read" in capi.ABI_SYMBOLS
    assert hasattr(capi.Context, "bound_pdb_set")
