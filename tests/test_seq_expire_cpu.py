"""bs_seq_expire on the CPU: the two statements of tests/seq_expire_ref.py held against each other on seeded scenes, hand known answers
(tests/golden/seq_expire_hand_kats.json), and the host-side list check (csrc/bs_seq_expire_list.hpp) compiled alone under ASan + UBSan.
No GPU."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import naive_ref as nv
import seq_expire_ref as ser
import seq_obj_replay as sor
from test_seq_oracle_pin import _with_waiting

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEEDS = range(240)


def scene(seed):
    """the families of tests/test_seq_oracle_pin.py (groups enter with waiting pods of earlier cycles, some phases closed) plus a crowded
    one: two to four nodes, so that several waiting pods — of one gang and of several — share a node"""
    if seed % 4 == 0:
        return _with_waiting(seed)
    if seed % 4 == 1:
        return _with_waiting(seed, n_nodes=int(6 + seed % 7), n_groups=int(2 + seed % 4), n_pods=int(20 + seed % 17), edge=False)
    if seed % 4 == 2:
        return _with_waiting(seed, n_nodes=int(3 + seed % 5), n_groups=3, n_pods=30, n_scalars=seed % 3, edge=True)
    return _with_waiting(seed, n_nodes=int(2 + seed % 3), n_groups=int(3 + seed % 3), n_pods=36, n_scalars=1 + seed % 2, edge=True)


def run_scene(orc, soa, seed):
    """one scene through both statements -> the property counters of this scene"""
    sc, closed = scene(seed)
    rng = np.random.default_rng(seed + 5)
    obj = sor.replay(sc, closed, scalar_names=sc["names"])
    nodes, fit, groups, pods, gidx = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], sc["denied"], sc["permitted"])
    for nm in closed:
        groups.flags[gidx[nm]] |= soa.GROUP_PHASE_CLOSED
    s = orc.seq_replay(nodes, fit, groups, pods, soa.STAGE_PREFILTER)
    wait, created = ser.waiting_after_pass(nodes, fit, groups, pods, s)
    st = ser.State(s["nodes"].requested, s["nodes"].requested_present, s["groups"].matched, s["groups"].flags, wait)
    names = list(sc["cache"].keys())
    G = len(names)
    deny = bool(seed % 2)
    use_all = seed % 3 == 0
    if use_all:
        glist = sorted({int(pods.group[i]) for i in np.nonzero(wait >= 0)[0]})
    else:
        glist = [int(g) for g in rng.permutation(G)[: int(rng.integers(0, G + 1))]]
    # ---- properties of the scene, counted on the array model before it changes
    wpods = [int(i) for i in np.nonzero(wait >= 0)[0] if int(pods.group[i]) in glist]
    on_node = {}
    for i in wpods:
        on_node.setdefault(int(wait[i]), []).append(int(pods.group[i]))
    S = nodes.lanes - 4
    prop = dict(
        several_on_one_node=any(len(v) > 1 for v in on_node.values()),
        two_gangs_on_one_node=any(len(set(v)) > 1 for v in on_node.values()),
        closed_gang_late_members=any(int(pods.group[i]) in set(s["released_group"].tolist()) and s["groups"].flags[int(pods.group[i])] & soa.GROUP_PHASE_CLOSED
                                     for i in wpods),
        key_created_by_assume=any((i, sc_) in created for i in wpods for sc_ in range(S)),
        negative_lane=any(int(pods.req[j, i]) < 0 and (j < 3 or (int(pods.req_present[i]) >> (j - 4)) & 1) for i in wpods for j in range(nodes.lanes) if j != 3),
    )
    res = ser.expire(st, pods, groups=None if use_all else glist, deny=deny, all=use_all)
    prop["group_earlier"] = bool(np.any(res["group_earlier"] > 0))
    # ---- the object level, same groups
    per = ser.expire_objects(obj["op"], sc, [names[g] for g in glist], deny=deny, scalar_names=sc["names"])
    assert res["group"].tolist() == glist
    assert res["group_pods"].tolist() == [len(rows) for rows, _ in per], f"seed {seed}"
    assert res["group_earlier"].tolist() == [e for _, e in per], f"seed {seed}"
    assert list(zip(res["pod"].tolist(), res["node"].tolist())) == [r for rows, _ in per for r in rows], f"seed {seed}"
    on = ser.object_nodes_soa(obj["op"], sc)
    assert np.array_equal(on.requested_present, st.requested_present), f"seed {seed}: node keys"
    assert np.array_equal(on.requested[:4], st.requested[:4]), f"seed {seed}: fixed lanes"
    for sc_ in range(S):
        has = ((st.requested_present >> sc_) & 1) != 0
        assert np.array_equal(on.requested[4 + sc_][has], st.requested[4 + sc_][has]), f"seed {seed}: scalar lane {sc_}"
    op = obj["op"]
    assert [op.cache[nm].matched for nm in names] == st.matched.tolist(), f"seed {seed}: matched"
    assert [op.last_denied.get(nm, op.now) is not None for nm in names] == [bool(f & soa.GROUP_DENIED) for f in st.flags], f"seed {seed}: deny list"
    assert [bool(op.cache[nm].scheduled) for nm in names] == [bool(f & soa.GROUP_SCHEDULED_LATCH) for f in st.flags], f"seed {seed}: the latch stays"
    # a second expire of the same groups forgets nothing and changes nothing
    before = (st.requested.copy(), st.matched.copy(), st.flags.copy())
    again = ser.expire(st, pods, groups=None if use_all else glist, deny=deny, all=use_all)
    assert again["n_pods"] == 0 and np.array_equal(before[0], st.requested) and np.array_equal(before[1], st.matched) and np.array_equal(before[2], st.flags)
    assert not np.any(again["group_earlier"]) and not np.any(again["group_pods"])
    return prop


def test_object_level_equals_array_level_and_scenes_cover_the_cases(orc, soa):
    total = {}
    for seed in SEEDS:
        for k, v in run_scene(orc, soa, seed).items():
            total[k] = total.get(k, 0) + int(bool(v))
    print(total)
    assert len(SEEDS) >= 200
    for k in ("several_on_one_node", "two_gangs_on_one_node", "group_earlier", "closed_gang_late_members", "key_created_by_assume", "negative_lane"):
        assert total[k] >= 1, (k, total)


def _kats():
    return json.load(open(os.path.join(HERE, "golden", "seq_expire_hand_kats.json")))["cases"]


@pytest.mark.parametrize("case", _kats(), ids=lambda c: c["name"])
def test_hand_known_answers(case):
    """scenes small enough to do by hand; the expected values were written down from the reference lines each case cites, not from a run"""
    assert case["cites"]
    L = len(case["requested"])
    pods = nv.soa.Pods(np.array(case["pod_group"], np.int32), np.array(case["pod_req"], np.int64).reshape(L, -1), np.array(case["pod_req_present"], np.uint32),
                       np.zeros(len(case["pod_group"]), np.uint32), np.zeros(len(case["pod_group"]), np.uint64), np.zeros(len(case["pod_group"]), np.uint8))
    st = ser.State(np.array(case["requested"], np.int64).reshape(L, -1), np.array(case["requested_present"], np.uint32), np.array(case["matched"], np.uint32),
                   np.array(case["flags"], np.uint8), np.array(case["wait_node"], np.int32))
    res = ser.expire(st, pods, groups=case.get("groups"), deny=case["deny"], all=case["all"])
    e = case["expect"]
    for k in ("group", "group_pods", "group_earlier", "pod", "node"):
        assert res[k].tolist() == e[k], k
    assert st.requested.tolist() == e["requested"] and st.requested_present.tolist() == e["requested_present"]
    assert st.matched.tolist() == e["matched"] and st.flags.tolist() == e["flags"] and st.wait_node.tolist() == e["wait_node"]


def test_list_check_under_sanitizers(tmp_path):
    """csrc/bs_seq_expire_list.hpp compiled alone with tests/native/seq_expire_list_main.cpp under ASan + UBSan, against the rule in Python"""
    exe = str(tmp_path / "seq_expire_list")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "seq_expire_list_main.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(23)
    lines, want = [], []
    for _ in range(400):
        g, count = int(rng.integers(0, 9)), int(rng.integers(0, 7))
        null = int(rng.random() < 0.25)
        flags = int(rng.choice([0, 1, 2, 3, 4, 8, 0x80000001]))
        lst = rng.integers(0, g + 2, size=count).tolist() if rng.random() < 0.5 else rng.permutation(max(g, 1))[:count].tolist()
        count = len(lst)
        lines.append(" ".join(map(str, [g, flags, null, count, *lst])))
        if flags & ~3:
            code = 1
        elif flags & 2:
            code = 2 if (not null or count) else 0
        elif null:
            code = 3
        elif any(x >= g for x in (lst[: g + 1] if count > g else lst)):
            code = 4
        elif count > g:
            code = 5
        elif len(set(lst)) != len(lst):
            code = 5
        else:
            code = 0
        want.append(code)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == want
    assert all(want.count(c) >= 5 for c in range(6)), [want.count(c) for c in range(6)]
    # a count far above g with every index in range: answered "twice" without a copy of the list (the driver repeats the given entries)
    out = subprocess.run([exe], input="3 0 0 3000000000 big 0 1 2 1\n3 0 0 3000000000 big 0 1 2 3\n", capture_output=True, text=True, check=True).stdout.split()
    assert out == ["5", "4"]


def test_the_expire_kernels_use_no_scratch_and_the_pass_has_its_unit_to_itself():
    """k_se_sum<S> / k_se_nodes<S>, S = 0..12, and the four lane-free kernels: no scratch; all of them come from tu_seq_expire.hip, a unit
    other than the one that emits k_seq_pass (profiles/seq_expire_isa_diff.txt says why)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources()
    res = {k: v for k, v in all_k.items() if "k_se_" in k}
    assert len(res) == 30, sorted(res)
    assert sum("k_se_sum" in k for k in res) == 13 and sum("k_se_nodes" in k for k in res) == 13
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
    units = {v["unit"] for v in res.values()}
    assert len(units) == 1 and units.isdisjoint({v["unit"] for k, v in all_k.items() if "k_seq_pass" in k})
