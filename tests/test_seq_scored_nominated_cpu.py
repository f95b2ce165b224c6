"""CPU tests of bs_seq_run_scored_nominated's rule (include/bsched.h, rule SP, D8, SP1, SP2): the object-level model
tests/seq_scored_nominated_ref.py against its second statement from arrays (tests/seq_scored_nominated_soa.py) on every scene the GPU tests
run, the two reductions on the parents' full scene sets — zero weights are seq_nominated_ref.replay, no rows are seq_scored_ref.replay —,
the hand-derived answers (tests/golden/seq_scored_nominated_hand_kats.json), the census of hazards over the GPU scene set, and where the new
kernels sit in the build.  No GPU: nothing here creates a context."""
import importlib
import os
import sys

import numpy as np
import pytest

import seq_nominated_ref as snr
import seq_nominated_scenes as sns
import seq_scored_nominated_ref as spr
import seq_scored_nominated_scenes as sps
import seq_scored_nominated_soa as spsoa
import seq_scored_ref as ssr
import seq_scored_scenes as sss
import seq_soa_ref as ssoa
from test_gpu_seq import assert_groups_equal

bsa = importlib.import_module("batch-scheduler_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ = ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods")
END = ("matched", "status_scheduled", "latch", "closed", "denied")
KATS = sps.load_kats()


def _scene(case):
    kind = case[0]
    if kind == "parity":
        return sps.parity_scene(*case[1:])
    if kind == "lean":
        return sps.lean_scene(*case[1:])
    if kind == "kat":
        return sps.kat_scene(KATS[case[1]])
    if kind == "border":
        return sps.border_scene(case[1], sss.WEIGHTS[case[2]])
    return dict(waves=sps.waves_scene)[kind]()


# the scenes the GPU tests run (the walk over 32 838 nodes is held by its own assertions below: the array model would take minutes on it)
CASES = ([("parity",) + c for c in sps.PARITY] + [("lean",) + c for c in sps.LEAN] + [("kat", i) for i in range(len(KATS))]
         + [("border", n, w) for n in (65, 513) for w in range(len(sss.WEIGHTS))] + [("waves",)])


# ---- the two statements of rule SP ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_the_object_model_is_the_array_model(case, orc, soa):
    scn = _scene(case)
    model = sps.model(scn)
    nodes, fit, groups, pods, owner_ids, rows = sps.to_soa(scn)
    ch = spsoa.ScoredNominatedChoice(rows, scn["priority"], scn["own_id"], scn["weights"], pods.p)
    got = ssoa.seq_pass(orc, nodes, fit, groups, pods, -1, ch)
    for k in SEQ + ("assumed",):
        assert got[k].tolist() == list(model[k]), f"{case}: {k}"
    assert ch.total.tolist() == model["total"] and ch.n_fit.tolist() == model["n_fit"], f"{case}: totals and candidate counts"
    en, eg, wait = spr.end_state_soa(model, scn["sc"], soa, dict(owner_ids))
    assert np.array_equal(got["nodes"].requested, en.requested) and np.array_equal(got["nodes"].requested_present, en.requested_present), f"{case}: node requests"
    assert_groups_equal(got["groups"], eg, soa, str(case))
    assert np.array_equal(got["wait_node"], wait), f"{case}: the pods that wait at Permit"
    assert sorted(ch.consumed) == model["consumed"], f"{case}: consumed rows"
    assert ch.live_ids().tolist() == [o.id for o in model["nominees"]], f"{case}: surviving rows"


# ---- SP1: zero weights are rule S ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,m", sns.PARITY, ids=[f"{s}-N{n}-m{m}" for s, n, m in sns.PARITY])
def test_sp1_zero_weights_are_the_nominated_model(seed, n, m):
    scn = sns.parity_scene(seed, n, m)
    a = spr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], (0, 0, 0), scalar_names=scn["names"])
    b = snr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], scalar_names=scn["names"])
    for k in SEQ + END + ("assumed", "consumed"):
        assert a[k] == b[k], (seed, k)
    assert [o.id for o in a["nominees"]] == [o.id for o in b["nominees"]], seed
    assert all(t == 0 for t in a["total"]) and a["hazards"]["b"] == 0, "every candidate ties at 0: the first member of C"
    assert sum(a["n_fit"]) > 0


# ---- SP2: no rows are rule P ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sss.SEEDS)
def test_sp2_no_rows_are_the_scored_model(seed):
    sc = sss.make(seed)
    w = sss.WEIGHTS[seed % len(sss.WEIGHTS)]
    prio = np.random.default_rng(seed).integers(-3, 40, size=len(sc["pods"]))
    a = spr.replay(sc, [], prio, None, w, scalar_names=sc["names"])
    b = ssr.replay(sc, w, scalar_names=sc["names"])
    for k in SEQ + END + ("assumed", "total", "n_fit"):
        assert a[k] == b[k], (seed, k)
    assert a["consumed"] == [] and a["nominees"] == [] and not any(a["hazards"][c] for c in "acdefghjk")


# ---- the hand-derived answers --------------------------------------------------------------------------------------------------------------
def test_the_golden_file_has_one_scene_per_hazard():
    assert [k["name"] for k in KATS] == list(spr.HAZARDS)
    assert all(3 <= len(k["nodes"]) <= 4 for k in KATS)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_hand_answers(kat):
    scn = sps.kat_scene(kat)
    model = sps.model(scn)
    assert model["assumed"] == kat["expect_node"], kat["why"]
    assert model["total"] == kat["expect_total"] and model["n_fit"] == kat["expect_n_fit"], kat["why"]
    assert [o.id for o in model["nominees"]] == kat["expect_rows"], kat["why"]
    assert model["hazards"][kat["name"]] >= 1, f"scene {kat['name']} shows its hazard: {model['hazards']}"


def test_d8_the_hand_scene_turns_when_rows_enter_the_score():
    """scene j once more with the row added to the node's own requests (what ranking by R + rows would read): the other node wins"""
    kat = next(k for k in KATS if k["name"] == "j")
    scn = sps.kat_scene(kat)
    row = scn["nominees"][0]
    scn["sc"]["nodes"][row.node].requested.MilliCPU += row.req.MilliCPU
    moved = ssr.replay(scn["sc"], scn["weights"])
    assert moved["assumed"] == [1] and kat["expect_node"] == [0]


# ---- the census of the GPU scene set ---------------------------------------------------------------------------------------------------------
def test_the_gpu_scene_set_meets_every_hazard():
    seen = {c: 0 for c in spr.HAZARDS + spr.EXTRA}
    placed = consumed = 0
    for case in [("parity",) + c for c in sps.PARITY]:
        md = sps.model(_scene(case))
        for c in seen:
            seen[c] += md["hazards"][c]
        placed += sum(1 for a in md["assumed"] if a >= 0)
        consumed += len(md["consumed"])
    assert all(seen[c] >= 1 for c in spr.HAZARDS), seen
    assert seen["a"] >= 100 and seen["b"] >= 100 and seen["e"] >= 100 and seen["g"] >= 50 and seen["h"] >= 100 and seen["j"] >= 50 and seen["k"] >= 50, seen
    assert placed >= 1000 and consumed >= 50, (placed, consumed)
    assert {(n, S) for _, n, _, S in sps.PARITY} == {(n, S) for n in sps.EDGE_N for S in sps.LANES} and {m for _, _, m, _ in sps.PARITY} == set(sps.ROWS)


@pytest.mark.parametrize("seed,n,m,S", sps.LEAN, ids=[f"{s}-N{n}-m{m}-S{S}" for s, n, m, S in sps.LEAN])
def test_the_lean_scenes_let_a_scalar_row_sum_and_the_key_rule_decide(seed, n, m, S):
    scn = sps.lean_scene(seed, n, m, S)
    assert len(scn["names"]) == S and any(o.req.ScalarResources for o in scn["nominees"])
    hz = sps.model(scn)["hazards"]
    assert hz["s"] >= 1, f"a row's scalar lane turns a node away: {hz}"
    assert hz["i"] >= 1, f"a row brings a scalar key the node's requests lack: {hz}"


def test_built_scenes_do_what_their_names_say():
    walks = sps.model(sps.walks_scene())
    W = sss.WALK
    assert walks["assumed"][1] == W and walks["assumed"][3] == W and walks["assumed"][5] == W - 1, walks["assumed"]
    assert walks["n_fit"] == [2, 2, 2, 2, 2, 3] and walks["hazards"]["g"] >= 1, "the tie across the two tile walks goes to 32 768 first, to 32 767 for the last pod"
    waves = sps.model(sps.waves_scene())
    # tile 65 lane 5, tile 66 lanes 1 and 9 tie (total 175) and the lowest index is behind the row for priority 5; a second pod on a node gives 162
    t64, t65, t66a, t66b = 64 * 64 + 5, 65 * 64 + 5, 66 * 64 + 1, 66 * 64 + 9
    assert waves["assumed"] == [t66a, t66b, t65, t64, t65, t66a] and waves["total"] == [175, 175, 175, 162, 162, 162], (waves["assumed"], waves["total"])
    assert waves["n_fit"] == [4, 4, 5, 4, 5, 4]
    for n in (65, 513):
        for w in sss.WEIGHTS:
            md = sps.model(sps.border_scene(n, w))
            assert md["hazards"]["h"] >= 1 and min(md["n_fit"]) >= 1, (n, w)
        md = sps.model(sps.border_scene(n, (1, 0, 1)))
        assert {n - 2, n - 1} <= set(md["assumed"]), "both sides of the border win under least requested + balanced"
        md = sps.model(sps.border_scene(n, (0, 1, 0)))
        assert n - 3 in md["assumed"], "the fullest node in front of the border wins under most requested"


# ---- where the new kernels sit --------------------------------------------------------------------------------------------------------------
def test_thirteen_instantiations_without_scratch_in_a_unit_of_their_own():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources(bsa.build.build())
    sp = {k: v for k, v in all_k.items() if "k_seq_sp" in k}
    assert len(sp) == 13, sorted(sp)                                              # 0 .. 12 scalar lanes, no generic-lane one (bs_seq.hpp)
    assert all(v["scratch"] == 0 and v["vgpr"] <= 256 for v in sp.values()), sp   # 512 threads on one CU: two waves per SIMD, 256 VGPRs
    units = {v["unit"] for v in sp.values()}
    assert len(units) == 1 and units.isdisjoint({v["unit"] for k, v in all_k.items() if k not in sp}), "nothing but the thirteen kernels in tu_seq_score_nom.hip"
    assert "tu_seq_score_nom.hip" in bsa.build.SOURCES
    summary = open(os.path.join(ROOT, "profiles", "seq_scored_nominated_isa_diff.txt")).read()
    for k in all_k:
        if ("k_seq_pass" in k or "k_seq_scored" in k):
            assert any(line.startswith("same " + k + " ") for line in summary.splitlines()), k
