"""The hand-derived answers of tests/golden/seq_hand_kats.json on the CPU: three models, one answer (orc.seq_replay, the object replay of
tests/seq_obj_replay.py, the SoA pass of tests/seq_soa_ref.py), the device path every scene is meant to reach (seq_hand_scenes.hazards),
and the set's power to tell a wrong pass from the right one: every single-rule mutant of seq_soa_ref.MUTANTS disagrees with at least one
hand answer.  The answers come from core.go and batchscheduler.go, not from a run of any of the three models."""
import numpy as np
import pytest

import seq_hand_scenes as shs
import seq_obj_replay as sor
import seq_soa_ref as ssoa

SCENES = shs.load()
DEVICE = [k for k in SCENES if not k.get("cpu_only")]
PASSES = [(k, j) for k in DEVICE for j in range(len(k["passes"]))]
PASS_IDS = [f"{k['name']}-pass{j}" if len(k["passes"]) > 1 else k["name"] for k, j in PASSES]


def assert_record(got, s, soa, where):
    """a model's record (the oracle's dict) against the hand record, field by field"""
    for f in ("pf_code", "pf_first_k", "pf_leader", "pod_node"):
        assert np.asarray(got[f]).tolist() == s[f].tolist(), f"{where}: {f}"
    n = len(s["released_group"])
    assert int(got["n_released"]) == s["n_released"], f"{where}: n_released"
    assert np.asarray(got["released_group"]).tolist()[:n] == s["released_group"].tolist(), f"{where}: gangs in release order"
    assert [int(v) & 0xFFFFFFFF for v in np.asarray(got["released_pods"]).tolist()[:n]] == s["released_pods"].tolist(), f"{where}: pods per gang"
    assert np.array_equal(got["nodes"].requested, s["nodes"].requested), f"{where}: requested"
    assert np.array_equal(got["nodes"].requested_present, s["nodes"].requested_present), f"{where}: requested keys"
    g, x = got["groups"], s["groups"]
    assert g.matched.tolist() == x.matched.tolist(), f"{where}: matched"
    assert g.status_scheduled.tolist() == x.status_scheduled.tolist(), f"{where}: Status.Scheduled"
    assert g.flags.tolist() == x.flags.tolist(), f"{where}: latch / closed / denied"
    if "assumed" in got:
        assert np.asarray(got["assumed"]).tolist() == s["assumed"].tolist(), f"{where}: the node every pod is assumed on"


def test_the_file_holds_what_the_issue_asks_for():
    a, b = [k for k in SCENES if k["kind"] == "A"], [k for k in SCENES if k["kind"] == "B"]
    assert len(a) >= 16 and len(b) >= 12 and len(SCENES) >= 28, (len(a), len(b))
    assert len([k for k in SCENES if k.get("cpu_only")]) <= shs.CPU_ONLY_MAX and len(DEVICE) >= 28
    for k in a:
        assert len(k["nodes"]) <= 4 and all(len(ps["pods"]) <= 12 for ps in k["passes"]), k["name"]
    for k in SCENES:
        assert len(k["nodes"]) <= 65 + 1 and all(len(ps["pods"]) <= 515 for ps in k["passes"]), k["name"]


def test_the_loader_refuses_unknown_fields():
    with pytest.raises(AssertionError, match="unknown fields"):
        shs._expand([{"alloc": {}, "colour": 1}], shs.NODE_FIELDS, "x")
    with pytest.raises(AssertionError, match="unknown fields"):
        shs._known({"pf_code": [], "pf_codes": []}, shs.EXPECT_FIELDS, "x")


@pytest.mark.parametrize("k,j", PASSES, ids=PASS_IDS)
def test_three_models_one_answer(k, j, orc, soa):
    s = shs.expected(k, j)
    nodes, fit, groups, pods = shs.to_soa(k, j)
    leader = int(k["passes"][j].get("carry_leader", -1))
    models = k.get("models", ["orc", "obj", "soa"])
    if "orc" in models:
        c = orc.seq_replay(nodes, fit, groups, pods, s["stages"], leader=leader)
        assert_record(c, s, soa, f"{k['name']} pass {j}: orc.seq_replay")
        if s["stages"] & soa.BATCH_FILTER_DENY:
            assert np.asarray(c["last_permitted"]).tolist() == s["last_permitted"].tolist()
    if "soa" in models and s["stages"] == soa.STAGE_PREFILTER:
        assert_record(ssoa.seq_pass(orc, nodes, fit, groups, pods, leader, ssoa.first_fit), s, soa, f"{k['name']} pass {j}: seq_soa_ref.seq_pass")
    if "obj" in models and leader < 0:                          # (the object replay has no stale leader to carry in)
        sc, closed = shs.objects(k, j)
        filt = bool(s["stages"] & soa.STAGE_FILTER)
        o = sor.replay(sc, closed, run_filter=filt, filter_deny=filt, scalar_names=sc["names"])
        where = f"{k['name']} pass {j}: seq_obj_replay"
        for f in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods"):
            assert list(o[f]) == s[f].tolist(), f"{where}: {f}"
        x = s["groups"]
        assert o["matched"] == x.matched.tolist() and o["status_scheduled"] == x.status_scheduled.tolist(), where
        for name, bit in (("latch", soa.GROUP_SCHEDULED_LATCH), ("closed", soa.GROUP_PHASE_CLOSED), ("denied", soa.GROUP_DENIED)):
            assert o[name] == [bool(f & bit) for f in x.flags], f"{where}: {name}"
        if filt:
            assert o["last_permitted"] == s["last_permitted"].tolist(), where
        lane = o["op"].nodes
        assert [n.requested.MilliCPU for n in lane] == s["nodes"].requested[0].tolist(), f"{where}: cpu requested"
        assert [n.requested.AllowedPodNumber or n.pod_count for n in lane] == s["nodes"].requested[3].tolist(), f"{where}: pods lane"


@pytest.mark.parametrize("k", [k for k in SCENES if k.get("cpu_only")], ids=lambda k: k["name"])
def test_clock_scenes_on_the_object_model(k):
    """the rules one clockless pass cannot state (the scene's cpu_only field says which): timed calls on oracle/naive_seq.SeqOperation, every
    answer derived by hand"""
    import naive_ref as nv
    sc, closed = shs.objects(k)
    op = sor.build_operation(sc, closed)
    for n, st in enumerate(k["steps"]):
        op.set_time(st["t"])
        pod = nv.Pod(st["uid"], st["group"], dict(st.get("req", {"cpu": 1000})))
        x, where = st["expect"], f"{k['name']} step {n}"
        if st["op"] == "permit":
            ready, code = op.permit(pod, st["pod_name"], st["node"])
            live = len(op.cache[st["group"]].matched_pod_nodes.live(op.now))
            assert (ready, code, live) == (x["ready"], x["code"], x["live"]), where
        elif st["op"] == "prefilter":
            code, fk = op.prefilter(pod)
            assert (code, fk) == (x["code"], shs.FIRST_K.get(x["first_k"], x["first_k"])), where
        else:
            assert op.filter(pod, st["node"]) == (x["fl"], x["fn"]), where


def test_every_scene_reaches_its_hazard_and_every_hazard_is_reached(capsys):
    total = dict.fromkeys(shs.COUNTERS + shs.STRUCTURAL, 0)
    for k in DEVICE:
        mine = dict.fromkeys(total, 0)
        for j in range(len(k["passes"])):
            for name, v in shs.hazards(k, j).items():
                mine[name] += v
        if k["hazard"] != "none":
            assert mine[k["hazard"]] > 0, f"{k['name']} does not reach {k['hazard']}: {mine}"
        for name, v in mine.items():
            total[name] += v
    with capsys.disabled():
        print("\nhazard counters over the device-runnable scenes:", total)
    assert all(v > 0 for v in total.values()), total


def test_list_scenes_sit_at_the_list_size():
    """511 and 512 waiting pods release from the list, 513 overflow it"""
    by = {k["name"]: shs.hazards(k) for k in DEVICE if k["name"].startswith("list_5")}
    assert [by[n]["list_valid"] for n in ("list_511", "list_512", "list_513")] == [1, 1, 0]
    assert [by[n]["list_overflowed"] for n in ("list_511", "list_512", "list_513")] == [0, 0, 1] and by["list_513"]["chain_walked"] == 1


def _disagrees(got, s, soa):
    try:
        assert_record(got, s, soa, "")
    except AssertionError:
        return True
    return False


def test_every_mutant_is_killed_by_a_hand_answer(orc, soa, capsys):
    cases = [(k, j, shs.expected(k, j), shs.to_soa(k, j)) for k, j in PASSES if shs.stages_of(k) == soa.STAGE_PREFILTER and len(k["passes"][j]["pods"]) <= 64
             and "soa" in k.get("models", ["soa"]) and len(k["groups"]) < 100]
    for k, j, s, (nodes, fit, groups, pods) in cases:
        leader = int(k["passes"][j].get("carry_leader", -1))
        assert not _disagrees(ssoa.seq_pass(orc, nodes, fit, groups, pods, leader, ssoa.first_fit), s, soa), f"the pass itself misses {k['name']}"
    killers = {}
    for m in ssoa.MUTANTS:
        for k, j, s, (nodes, fit, groups, pods) in cases:
            leader = int(k["passes"][j].get("carry_leader", -1))
            if _disagrees(ssoa.seq_pass(orc, nodes, fit, groups, pods, leader, ssoa.first_fit, mutate=m), s, soa):
                killers.setdefault(m, []).append(k["name"])
    with capsys.disabled():
        print()
        for m in ssoa.MUTANTS:
            print(f"mutant {m:22s} killed by {killers.get(m, ['NOBODY'])[0]} (+{max(len(killers.get(m, [])) - 1, 0)} more)")
    assert not [m for m in ssoa.MUTANTS if m not in killers], "a mutant no scene kills means a scene is missing"
