"""The pass model over SoA (tests/seq_soa_ref.py) held against the statements of each rule that exist already, no GPU:

  first fit  orc.seq_replay (the C oracle) on the state in front of every pass of every plan of tests/world_ref.py
  rule S     seq_nominated_ref.replay (objects) on the scene set of tests/seq_nominated_scenes.py — the GPU parity set and the hand-derived
             scenes of tests/golden/seq_nominated_hand_kats.json — through its to_soa
  rule P     seq_scored_ref.replay (objects) on seq_scored_scenes.PARITY and PARITY_MAX, the hand scenes of
             tests/golden/seq_scored_hand_kats.json and out_of_domain()"""
import numpy as np
import pytest

import seq_nominated_ref as snr
import seq_nominated_scenes as sns
import seq_scored_ref as ssr
import seq_scored_scenes as sss
import seq_soa_ref as ssoa
import world_ref as wf
from test_gpu_seq import assert_groups_equal

SEQ = ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods")


def test_the_flag_words_are_the_package_s(soa):
    assert (ssoa.GROUP_SCHEDULED_LATCH, ssoa.GROUP_PHASE_CLOSED) == (soa.GROUP_SCHEDULED_LATCH, soa.GROUP_PHASE_CLOSED)
    assert ssoa.NOM_NONE == snr.NOM_NONE


# ---- first fit: the C oracle, from every state a plan reaches -------------------------------------------------------------------------------
PLANS = [("plan", s) for s in range(wf.SEEDS)] + [("plan_nom", s) for s in range(wf.NOM_SEEDS)]


@pytest.mark.parametrize("which,seed", PLANS, ids=[f"{w}-{s}" for w, s in PLANS])
def test_first_fit_is_the_c_oracle_on_every_pass_of_every_plan(which, seed, orc, soa):
    sc, steps = getattr(wf, which)(seed, orc)
    w = wf.world_of(orc, sc)
    passes = 0
    for i, (kind, args, refused) in enumerate(steps):
        if kind in ("pass", "pass_nom", "pass_scored") and not refused:
            where = f"{which}({seed}) step {i}"
            c = orc.seq_replay(w.nodes().copy(), w.fit(), w.groups, w.pods, soa.STAGE_PREFILTER, leader=w.leader)
            got = ssoa.seq_pass(orc, w.nodes(), w.fit(), w.groups, w.pods, w.leader, ssoa.first_fit)
            for k in SEQ + ("n_released", "leader"):
                assert np.array_equal(got[k], c[k]), f"{where}: {k}"
            assert np.array_equal(got["nodes"].requested, c["nodes"].requested), f"{where}: node requests"
            assert np.array_equal(got["nodes"].requested_present, c["nodes"].requested_present), f"{where}: node request keys"
            for col in wf.gl.COLUMNS:
                assert np.array_equal(getattr(got["groups"], col), getattr(c["groups"], col)), f"{where}: groups.{col}"
            wait, _ = wf.ser.waiting_after_pass(w.nodes().copy(), w.fit(), w.groups, w.pods, c)
            assert np.array_equal(got["wait_node"], wait), f"{where}: the pods that wait at Permit"
            passes += 1
        w.step(kind, args)
    assert passes >= 2, f"{which}({seed}) has {passes} passes"


# ---- rule S: the object model ---------------------------------------------------------------------------------------------------------------
NOM_CASES = [("parity",) + c for c in sns.PARITY] + [("kat", i) for i in range(len(sns.load_kats()))]


def _nom_scene(case):
    return sns.parity_scene(*case[1:]) if case[0] == "parity" else sns.kat_scene(sns.load_kats()[case[1]])


@pytest.mark.parametrize("case", NOM_CASES, ids=["-".join(str(x) for x in c) for c in NOM_CASES])
def test_rule_s_is_the_object_model(case, orc, soa):
    scn = _nom_scene(case)
    model = snr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], scalar_names=scn["names"])
    nodes, fit, groups, pods, owner_ids, rows = sns.to_soa(scn)
    ch = ssoa.NominatedChoice(rows, scn["priority"], scn["own_id"])
    got = ssoa.seq_pass(orc, nodes, fit, groups, pods, -1, ch)
    for k in SEQ + ("assumed",):
        assert got[k].tolist() == list(model[k]), f"{case}: {k}"
    en, eg, wait = snr.end_state_soa(model, scn["sc"], soa, dict(owner_ids))
    assert np.array_equal(got["nodes"].requested, en.requested) and np.array_equal(got["nodes"].requested_present, en.requested_present), f"{case}: node requests"
    assert_groups_equal(got["groups"], eg, soa, str(case))
    assert np.array_equal(got["wait_node"], wait), f"{case}: the pods that wait at Permit"
    assert sorted(ch.consumed) == model["consumed"], f"{case}: consumed rows"
    assert ch.live_ids().tolist() == [o.id for o in model["nominees"]], f"{case}: surviving rows"
    assert ch.blocked == model["blocked"], f"{case}: pods a row turned away from a node"


# ---- rule P: the object model ---------------------------------------------------------------------------------------------------------------
def _scored_cases():
    out = [(f"parity-{c[0]}", sss.parity_scene(*c), sss.WEIGHTS[i % len(sss.WEIGHTS)]) for i, c in enumerate(sss.PARITY)]
    out += [(f"max-{c[0]}", sss.parity_scene(*c), sss.WEIGHTS[(i + 3) % len(sss.WEIGHTS)]) for i, c in enumerate(sss.PARITY_MAX)]
    for k in sss.load_kats()["scenes"]:
        out += [(f"kat-{k['name']}-{wt}", sss.kat_scene(k), tuple(int(x) for x in wt.split(","))) for wt in k["expect"]]
    out += [(f"out_of_domain-{w}", sss.out_of_domain(), w) for w in sss.WEIGHTS]
    return out


def test_rule_p_is_the_object_model(orc, soa):
    cases = _scored_cases()
    differs = 0
    for name, sc, weights in cases:
        model = ssr.replay(sc, weights, scalar_names=sc["names"])
        nodes, fit, groups, pods, owner_ids = sss.to_soa(sc)
        ch = ssoa.ScoredChoice(weights, pods.p)
        got = ssoa.seq_pass(orc, nodes, fit, groups, pods, -1, ch)
        for k in SEQ + ("assumed",):
            assert got[k].tolist() == list(model[k]), f"{name}: {k}"
        assert ch.total.tolist() == model["total"] and ch.n_fit.tolist() == model["n_fit"], f"{name}: total, n_fit"
        en, eg, wait = ssr.end_state_soa(model, sc, soa, dict(owner_ids))
        assert np.array_equal(got["nodes"].requested, en.requested) and np.array_equal(got["nodes"].requested_present, en.requested_present), f"{name}: node requests"
        assert_groups_equal(got["groups"], eg, soa, name)
        assert np.array_equal(got["wait_node"], wait), f"{name}: the pods that wait at Permit"
        differs += model["hazards"]["a"] > 0
    assert 2 * differs >= len(cases), f"the choice differs from first fit in {differs} of {len(cases)} scenes"
