"""CPU: the node half of bs_bound_apply_ex (BS_BOUND_NODES) — the numpy model of tests/bound_apply_nodes_ref.py against the object-level
restatement that calls RemovePod / AddPod one entry at a time, on seeded scenes built around each rule; against the hand known answers
of tests/golden/bound_apply_nodes_hand_kats.json; and against the model of BS_PREEMPT_APPLY (tests/preempt_commit_ref.py): removing
exactly a plan's victims gives the node requests that model's APPLY leaves."""
import numpy as np
import pytest

import bound_apply_nodes_ref as bn
import bound_apply_ref as ba
import preempt_commit_ref as pc
from preempt_scenes import random_scene

SEEDS = range(360)


def _run(sc):
    a = bn.State(sc["bound"], sc["S"], sc["n"], sc["req"], sc["pres"])
    o = bn.ObjState(sc["bound"], sc["S"], sc["n"], sc["req"], sc["pres"])
    for step, (rem, ins) in enumerate(sc["steps"]):
        assert a.apply_ex(rem, ins) == o.apply_ex(rem, ins), step
        assert np.array_equal(a.req, o.req) and np.array_equal(a.pres, o.pres), f"{sc['kind']} step {step}: {a.req.tolist()} vs {o.req.tolist()}"
        assert sorted(o.live) == sorted(a.t.id.tolist())
    return a, o


def test_the_two_restatements_agree_on_seeded_scenes():
    assert len(SEEDS) >= 300
    seen = {k: 0 for k in bn.KINDS}
    wraps = 0
    for seed in SEEDS:
        sc = bn.scene(seed)
        _, o = _run(sc)
        seen[sc["kind"]] += 1
        wraps += o.wraps
    assert all(v >= 50 for v in seen.values()), seen
    assert wraps > 100, wraps


def test_the_scenes_hold_the_cases_they_are_named_for():
    """each kind's first step is the case, and it shows in the result the way the rule says"""
    for seed in range(60):
        sc = bn.scene(seed)
        S, n, kind = sc["S"], sc["n"], sc["kind"]
        rem, ins = sc["steps"][0]
        a = bn.State(sc["bound"], S, n, sc["req"], sc["pres"])
        o = bn.ObjState(sc["bound"], S, n, sc["req"], sc["pres"])
        before, bpres = a.req.copy(), a.pres.copy()
        a.apply_ex(rem, ins)
        o.apply_ex(rem, ins)
        if kind == "absent_on_node":                       # every key of the inserted pods: from 0, not from the lane's word
            _, ipres = ba.stored(ins, S)
            assert not bpres.any() and ipres.all()
            for k in np.unique(ins.node):
                on = ins.node == k
                assert a.pres[k] == (1 << S) - 1
                for s in range(S):
                    with np.errstate(over="ignore"):
                        assert a.req[4 + s, k] == ins.req[4 + s][on].sum()
        elif kind == "remove_only_key" and rem:
            i = rem[0]
            k, bits = int(sc["bound"].node[i]), int(sc["bound"].req_present[i]) & ((1 << S) - 1)
            assert ins is None and a.pres[k] == bpres[k] | bits
            for s in range(S):
                if (bits >> s) & 1:
                    base = int(before[4 + s, k]) if (int(bpres[k]) >> s) & 1 else 0
                    assert int(a.req[4 + s, k]) == bn._wrap(base - int(sc["bound"].req[4 + s, i]))
                else:
                    assert a.req[4 + s, k] == before[4 + s, k]
        elif kind == "wrap_and_return":
            assert o.wraps >= 2 and a.req[0, 0] != before[0, 0]
            rem2, ins2 = sc["steps"][1]
            a.apply_ex(rem2, ins2)
            o.apply_ex(rem2, ins2)
            assert o.wraps >= 4 and np.array_equal(a.req, before) and np.array_equal(a.req, o.req)      # back where it started
        elif kind == "whole_node":
            assert len(rem) >= 2 and not np.any(a.t.node == 0)
            assert a.req[3, 0] == before[3, 0] - len(rem)
            assert np.array_equal(a.req[:, 1:], before[:, 1:])
        elif kind == "inserts_only":
            k = n - 1
            assert not rem and not np.any(sc["bound"].node == k) and a.req[3, k] == before[3, k] + ins.b
            assert np.array_equal(a.req[:, :k], before[:, :k])


def test_hand_known_answers():
    kats = bn.hand_kats()
    assert len(kats) >= 10 and all(k["pins"] for k in kats)
    for sc in kats:
        S, n = sc["S"], sc["n"]
        bound, ins = bn.kat_entries(sc["bound"], S), bn.kat_entries(sc["insert"], S)
        for model in (bn.State, bn.ObjState):
            m = model(bound, S, n, sc["node_req"], sc["node_pres"])
            assert m.apply_ex(sc["remove"], ins, flags=sc["flags"]) == bound.b, sc["name"]
            assert m.req.tolist() == sc["expect_req"] and m.pres.tolist() == sc["expect_pres"], (sc["name"], model.__name__, m.req.tolist(), m.pres.tolist())


def test_errors_and_unknown_flags_change_nothing():
    sc = bn.scene(1)
    a = bn.State(sc["bound"], sc["S"], sc["n"], sc["req"], sc["pres"])
    a.apply_ex([0], None)
    req, pres, tab = a.req.copy(), a.pres.copy(), a.t.table()
    one = bn._entries(np.random.default_rng(1), [0], sc["S"])
    for rem, ins, flags in (([0], one, 1), ([1, 1], one, 1), ([a.t.ids], None, 1), ([1], one, 2), ([1], one, 3), ([], one, 0x80000000)):
        with pytest.raises(ba.ApplyError) as e:
            a.apply_ex(rem, ins, flags=flags)
        assert e.value.status == -1
        after = a.t.table()
        assert np.array_equal(a.req, req) and np.array_equal(a.pres, pres) and all(np.array_equal(tab[f], after[f]) for f in tab)
    many = bn._entries(np.random.default_rng(2), np.zeros(ba.MAX_PER_NODE + 1), sc["S"])
    with pytest.raises(ba.ApplyError) as e:
        a.apply_ex([], many)
    assert e.value.status == -5 and np.array_equal(a.req, req) and np.array_equal(a.pres, pres)


@pytest.mark.parametrize("seed,n,per,S", [(11, 6, (2, 9), 0), (12, 9, (3, 8), 2), (13, 5, (4, 12), 4), (14, 12, (2, 6), 1)])
def test_removing_a_plans_victims_is_what_preempt_apply_leaves(seed, n, per, S):
    sc = random_scene(seed, n, per, S, q=10, groups=0, flagged=0.0)
    cap = sc["bound"].b + 1
    prep = pc.CommitPrep(sc["nodes"], sc["bound"], S)
    exp = pc.commit_np(prep, sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"], sc["protected"], cap, apply=True)
    victims = pc.victim_ids(exp["res"])
    assert victims, "no victim: the comparison shows nothing"
    for model in (bn.State, bn.ObjState):
        m = model(sc["bound"], S, n, sc["nodes"].requested, sc["nodes"].requested_present)
        m.apply_ex(victims, None)
        assert np.array_equal(m.req, exp["req"]) and np.array_equal(m.pres, exp["pres"]), model.__name__
    a = bn.State(sc["bound"], S, n, sc["nodes"].requested, sc["nodes"].requested_present)
    a.apply_ex(victims, None)
    tab = a.t.table()
    assert np.array_equal(tab["id"], exp["bound_id"]) and np.array_equal(tab["node"], exp["bound_node"])
