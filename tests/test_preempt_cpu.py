"""CPU checks of the preemption restatements (tests/preempt_ref.py): the object-level one (core.go:203-260 and upstream's
selectVictimsOnNode / pickOneNodeForPreemption written out) against the numpy one on random scenes, both against the hand-derived
known answers of tests/golden/preempt_hand_kats.json (one scene per rule, each citing its line), and the helper the binding offers for
group_protected."""
import importlib

import numpy as np
import pytest

import preempt_ref as pr
from preempt_scenes import hand_kats, kat_scene, random_scene

bsa = importlib.import_module("batch-scheduler_amd")

FIELDS = ("node", "n_candidates", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start")


def _assert_same(a, b, where):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), f"{where}: {f}: {a[f]} vs {b[f]}"


def check_kat(res, sc, where):
    for i, e in enumerate(sc["expect"]):
        assert int(res["node"][i]) == e["node"], f"{where} [{i}]: node {res['node'][i]} != {e['node']}"
        assert int(res["n_candidates"][i]) == e["n_candidates"], f"{where} [{i}]: n_candidates"
        assert list(pr.victims_of(res, i)) == e["victims"], f"{where} [{i}]: victims {pr.victims_of(res, i)} != {e['victims']}"
        assert int(res["n_victims"][i]) == len(e["victims"])
        for f in ("top_priority", "priority_sum", "earliest_start"):
            if e[f] is not None:
                assert int(res[f][i]) == e[f], f"{where} [{i}]: {f} {res[f][i]} != {e[f]}"


@pytest.mark.parametrize("sc", hand_kats(), ids=lambda s: s["name"])
def test_hand_known_answers_both_restatements(sc):
    s = kat_scene(sc)
    cap = 8
    obj = pr.preempt_obj(s["nodes"], s["fit"], s["pods"], s["bound"], s["S"], s["pod_index"], s["priority"], s["protected"], cap)
    check_kat(obj, sc, f"object-level {sc['name']} ({sc['cite']})")
    nump = pr.preempt_np(pr.Prep(s["nodes"], s["bound"], s["S"]), s["fit"], s["pods"], s["pod_index"], s["priority"], s["protected"], cap)
    check_kat(nump, sc, f"numpy {sc['name']} ({sc['cite']})")


def test_every_policy_branch_is_covered_by_a_known_answer():
    names = {s["name"] for s in hand_kats()}
    for n in ("online_preempts_online", "offline_never_preempts_online", "online_preempts_offline", "online_refused_by_protected_gang",
              "victim_group_missing", "offline_same_gang_refused", "offline_other_gang_allowed", "offline_other_gang_protected",
              "refused_pod_drops_node_even_if_reprieved", "equal_priority_never_victim", "reprieve_in_importance_order",
              "pick_lowest_top_priority", "pick_lowest_priority_sum", "pick_fewest_victims", "pick_latest_earliest_start",
              "pick_lowest_index_on_full_tie", "zero_victims_win_lowest_index"):
        assert n in names


@pytest.mark.parametrize("S", [0, 1, 3])
@pytest.mark.parametrize("seed", range(6))
def test_object_level_equals_numpy_on_random_scenes(seed, S):
    per = [(0, 3), (2, 9), (5, 14)][seed % 3]
    sc = random_scene(1000 + seed, n=23 + 7 * seed, per_node=per, S=S, q=24)
    cap = 4
    obj = pr.preempt_obj(sc["nodes"], sc["fit"], sc["pods"], sc["bound"], S, sc["pod_index"], sc["priority"], sc["protected"], cap)
    nump = pr.preempt_np(pr.Prep(sc["nodes"], sc["bound"], S), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], cap)
    _assert_same(obj, nump, f"seed {seed} S {S}")


def test_random_scenes_exercise_every_outcome():
    """the random scenes are not degenerate: nodes chosen with and without victims, and preemptors with no node"""
    seen = set()
    for seed in range(6):
        sc = random_scene(1000 + seed, n=40, per_node=(2, 9), S=1, q=24)
        r = pr.preempt_np(pr.Prep(sc["nodes"], sc["bound"], 1), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], 4)
        seen |= {"none" if n < 0 else ("free" if v == 0 else "victims") for n, v in zip(r["node"], r["n_victims"])}
        seen |= {"overflow"} if np.any(r["n_victims"] > 4) else set()
    assert seen >= {"none", "free", "victims"}, seen


def test_group_protected_from_phases():
    capi = bsa.capi
    # bsh_phase: 0 "", 1 Pending, 2 Running, 3 PreScheduling, 4 Scheduling, 5 Scheduled, 6 Unknown, 7 Finished, 8 Failed
    assert list(capi.group_protected(range(9))) == [0, 0, 1, 0, 0, 1, 0, 0, 0]
    assert capi.group_protected([]).dtype == np.uint8


def test_make_bound_is_consistent_and_leaves_the_old_generators_alone():
    synth = bsa.synth
    bound, nodes = synth.make_bound(5, 50, 4, (0, 12), 2, unlisted=False)
    for j in (0, 1, 2):
        assert np.array_equal(np.bincount(bound.node, weights=bound.req[j], minlength=50).astype(np.int64), nodes.requested[j])
    assert np.array_equal(np.bincount(bound.node, minlength=50), nodes.requested[3])
    a = synth.make("tiny", "tail")
    b = synth.make("tiny", "tail")
    assert np.array_equal(a[0].requested, b[0].requested) and np.array_equal(a[3].req, b[3].req)
