"""CPU checks of the sequential preemption restatements (tests/preempt_commit_ref.py): the object-level one and the numpy one against
the hand-derived known answers of tests/golden/preempt_commit_hand_kats.json and against each other on random scenes; slot 0 equals
bs_preempt_run's answer for that preemptor alone; no bound pod is evicted twice; replaying a plan node by node, every nominee holds."""
import numpy as np
import pytest

import preempt_commit_ref as pc
import preempt_ref as pr
from preempt_commit_scenes import commit_kats, kat_commit_scene
from preempt_scenes import random_scene

FIELDS = ("node", "n_candidates", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start")


def check_commit_kat(got, sc, where):
    res = got["res"]
    for i, e in enumerate(sc["expect"]):
        assert int(res["node"][i]) == e["node"], f"{where} [{i}]: node {res['node'][i]} != {e['node']}"
        assert int(res["n_candidates"][i]) == e["n_candidates"], f"{where} [{i}]: n_candidates {res['n_candidates'][i]} != {e['n_candidates']}"
        assert list(pr.victims_of(res, i)) == e["victims"], f"{where} [{i}]: victims {pr.victims_of(res, i)} != {e['victims']}"
        assert int(res["n_victims"][i]) == e.get("n_victims", len(e["victims"])), f"{where} [{i}]: n_victims"
        for f in ("top_priority", "priority_sum", "earliest_start"):
            if e[f] is not None:
                assert int(res[f][i]) == e[f], f"{where} [{i}]: {f} {res[f][i]} != {e[f]}"
    st = sc["expect_state"]
    if st is not None:
        assert np.array_equal(np.asarray(got["req"]), np.array(st["req"], np.int64)), f"{where}: node requests {got['req'].tolist()}"
        assert np.array_equal(np.asarray(got["pres"]), np.array(st["pres"], np.uint32)), f"{where}: present bits"
        assert list(got["bound_id"]) == st["bound_id"] and list(got["bound_node"]) == st["bound_node"], \
            f"{where}: bound table {list(got['bound_id'])} / {list(got['bound_node'])}"


def _both(s, cap, apply, assume):
    obj = pc.commit_obj(s["nodes"], s["fit"], s["pods"], s["bound"], s["S"], s["pod_index"], s["priority"], s["protected"], cap, apply, assume)
    nump = pc.commit_np(pc.CommitPrep(s["nodes"], s["bound"], s["S"]), s["fit"], s["pods"], s["bound"], s["pod_index"], s["priority"],
                        s["protected"], cap, apply, assume)
    return obj, nump


@pytest.mark.parametrize("sc", commit_kats(), ids=lambda s: s["name"])
def test_hand_known_answers_both_restatements(sc):
    s = kat_commit_scene(sc)
    obj, nump = _both(s, s["cap"], s["apply"], s["assume"])
    check_commit_kat(obj, sc, f"object-level {sc['name']}")
    check_commit_kat(nump, sc, f"numpy {sc['name']}")


def test_known_answers_cover_the_rules():
    names = {s["name"] for s in commit_kats()}
    assert len(names) >= 12
    for n in ("two_equal_preemptors_one_victim", "nominee_fills_last_pod_slot", "nominee_fills_last_room", "eviction_leaves_room_for_a_victim_free_fit",
              "priority_overrides_caller_order", "equal_priorities_keep_caller_order", "victim_of_an_earlier_slot_is_not_counted_again",
              "scalar_key_introduced_by_a_nominee", "policy_still_refuses_after_evictions", "victim_cap_truncates_but_every_victim_is_evicted"):
        assert n in names


def commit_random_scene(seed, S, q=24, **kw):
    sc = random_scene(seed, S=S, q=q, p=3 * q, **kw)
    sc["pod_index"] = np.random.default_rng(seed).permutation(3 * q)[:q].astype(np.uint32)
    return sc


@pytest.mark.parametrize("S", [0, 1, 4])
@pytest.mark.parametrize("seed", range(5))
def test_object_level_equals_numpy_on_random_scenes(seed, S):
    per = [(0, 3), (2, 9), (5, 14)][seed % 3]
    sc = commit_random_scene(3000 + seed, S, n=23 + 7 * seed, per_node=per)
    for apply, assume in ((False, False), (True, False), (True, True)):
        obj, nump = _both(sc, 4, apply, assume)
        for f in FIELDS:
            assert np.array_equal(obj["res"][f], nump["res"][f]), f"seed {seed} S {S}: {f}"
        for f in ("req", "pres", "bound_id", "bound_node"):
            assert np.array_equal(obj[f], nump[f]), f"seed {seed} S {S} apply {apply} assume {assume}: {f}"


@pytest.mark.parametrize("seed", range(4))
def test_slot_zero_is_bs_preempt_runs_answer(seed):
    sc = commit_random_scene(3100 + seed, 1, n=40, per_node=(2, 9))
    _, nump = _both(sc, 4, False, False)
    i = int(pc.slot_order(sc["priority"])[0])
    one = pr.preempt_obj(sc["nodes"], sc["fit"], sc["pods"], sc["bound"], 1, sc["pod_index"][[i]], sc["priority"][[i]], sc["protected"], 4)
    for f in FIELDS:
        assert np.array_equal(one[f][0], nump["res"][f][i]), f


@pytest.mark.parametrize("seed", range(4))
def test_no_victim_twice_and_every_nominee_holds(seed):
    S = 2
    sc = commit_random_scene(3200 + seed, S, q=40, n=30, per_node=(3, 12))
    cap = 64
    _, nump = _both(sc, cap, False, False)
    res = nump["res"]
    vic = pc.victim_ids(res)
    assert len(vic) == len(set(vic))
    assert np.any(res["n_victims"] > 0)
    # replay node by node in slot order: requests after the earlier slots' victims and nominees
    b, pods = sc["bound"], sc["pods"]
    eff = sc["nodes"].requested.astype(np.int64).copy()
    for t in range(S):
        eff[4 + t] = np.where((sc["nodes"].requested_present >> np.uint32(t)) & 1, eff[4 + t], 0)
    al, ap = sc["nodes"].allocatable.astype(np.int64), sc["nodes"].allocatable_present.astype(np.int64)
    for i in pc.slot_order(sc["priority"]):
        k = int(res["node"][i])
        if k < 0:
            continue
        pi = int(sc["pod_index"][i])
        for v in pr.victims_of(res, i):
            assert int(b.node[v]) == k and int(b.priority[v]) < int(sc["priority"][i])
            eff[:3, k] -= b.req[:3, v]
            eff[3, k] -= 1
            for t in range(S):
                eff[4 + t, k] -= b.req[4 + t, v] if (int(b.req_present[v]) >> t) & 1 else 0
        assert pr.holds_np(al[:, k:k + 1], ap[k:k + 1], eff[:, k:k + 1], pods.req[:, pi].astype(np.int64), int(pods.req_present[pi]), S)[0], \
            f"preemptor {i} does not hold on node {k}"
        eff[:3, k] += pods.req[:3, pi]
        eff[3, k] += 1
        for t in range(S):
            eff[4 + t, k] += pods.req[4 + t, pi] if (int(pods.req_present[pi]) >> t) & 1 else 0
