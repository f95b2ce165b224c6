"""CPU checks of bs_preempt_commit_gang's restatements (tests/preempt_gang_ref.py): the object-level one (snapshot and restore) and the
defining property (the list without the voided runs' preemptors) against each other on seeded scenes and against the hand known
answers of tests/golden/preempt_gang_hand_kats.json; all needs 0 against bs_preempt_commit's restatement; the run rule; gang_order and
gang_need of the binding; and the host's run arrays (csrc/bs_preempt_gang_runs.hpp) compiled alone under ASan / UBSan."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import preempt_commit_ref as pc
import preempt_gang_paths as gp
import preempt_gang_ref as gr
import preempt_gang_scenes as gs
import preempt_pdb_ref as pp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _same(a, b, where):
    for f in pp.FIELDS:
        assert np.array_equal(a["res"][f], b["res"][f]), f"{where}: {f}\n{a['res'][f]}\n{b['res'][f]}"
    for f in gs.STATE + ("slot_voided", "group_placed"):
        assert np.array_equal(a[f], b[f]), f"{where}: {f}"


@pytest.mark.parametrize("sc", gs.gang_kats(), ids=lambda s: s["name"])
def test_hand_known_answers_both_restatements(sc):
    s = gs.kat_gang_scene(sc)
    check = dict(cap=s["cap"], apply=s["apply"], assume=s["assume"])
    gs.check_gang_kat(gs.expect_obj(s, **check), sc, f"object-level {sc['name']}")
    gs.check_gang_kat(gs.expect(s, **check), sc, f"defining property {sc['name']}")


def test_known_answers_cover_the_rules():
    seen = {}
    for sc in gs.gang_kats():
        s = gs.kat_gang_scene(sc)
        for k, v in gp.classify(s, s["cap"]).items():
            seen[k] = seen.get(k, 0) + v
    for k in ("voided_placed", "standing", "same_node", "revictim", "dirty_reuse", "over_cap", "run_of_one", "need_eq_placed", "need_gt_len", "run_at_end"):
        assert seen[k] > 0, (k, seen)


SEEDS = [(seed, S) for S in (0, 1, 4) for seed in range(40)]


@pytest.mark.parametrize("block", range(6))
def test_object_level_equals_defining_property_on_seeded_scenes(block):
    """240 scenes in six blocks (40 seeds x S in 0, 1, 4; plan only, apply, apply + assume, by turns); over each block both outcomes occur"""
    seen = dict(voided_placed=0, standing=0)
    for x, (seed, S) in enumerate(SEEDS[block::6] * 2):
        per = [(0, 3), (2, 9), (5, 14)][seed % 3]
        sc = gs.gang_scene(7000 + seed + 100 * S + 1000 * (x >= len(SEEDS[block::6])), n=5 + 3 * (seed % 7), per_node=per, S=S, q=20, groups=5,
                           share=0.3 if seed % 2 else 0.0)
        apply, assume = [(False, False), (True, False), (True, True)][x % 3]
        cap = (0, 1, 4)[seed % 3]
        a, b = gs.expect_obj(sc, cap, apply, assume), gs.expect(sc, cap, apply, assume)
        _same(a, b, f"seed {seed} S {S} apply {apply} assume {assume}")
        for r in a["trace"]:
            seen["voided_placed"] += r["voided"] and r["placed"] > 0
            seen["standing"] += not r["voided"]
    assert seen["voided_placed"] > 0 and seen["standing"] > 0, seen


@pytest.mark.parametrize("seed", range(6))
def test_all_needs_zero_is_the_plain_commit(seed):
    sc = gs.gang_scene(7300 + seed, n=17, per_node=(2, 9), S=seed % 3, q=24, groups=5, share=0.3)
    sc["need"][:] = 0
    for apply, assume in ((False, False), (True, True)):
        plain = pp.commit_pdb_obj(sc["nodes"], sc["fit"], sc["pods"], sc["bound"], sc["S"], sc["pod_index"], sc["priority"], sc["protected"], 4,
                                  sc["violating"], apply, assume)
        for got in (gs.expect_obj(sc, 4, apply, assume), gs.expect(sc, 4, apply, assume)):
            for f in pp.FIELDS:
                assert np.array_equal(got["res"][f], plain["res"][f]), f
            for f in gs.STATE:
                assert np.array_equal(got[f], plain[f]), f
            assert not got["slot_voided"].any() and not got["group_placed"].any()
    # without PDB bits the plain restatement of tests/preempt_commit_ref.py is the yardstick
    sc["violating"] = None
    plain = pc.commit_obj(sc["nodes"], sc["fit"], sc["pods"], sc["bound"], sc["S"], sc["pod_index"], sc["priority"], sc["protected"], 4, True, False)
    got = gs.expect_obj(sc, 4, True, False)
    for f in plain["res"]:
        assert np.array_equal(got["res"][f], plain["res"][f]), f


def test_run_rule():
    assert gr.runs_of([0, 0, 1, -1, 2, 2], [1, 0, 3]) == [(0, 1, 0), (4, 5, 2)]
    assert gr.runs_of([-2, -1, 5], [1]) == []                      # missing, ungrouped, and a group index beyond need[]
    assert gr.runs_of([0, 1, 0], [0, 2]) == [(1, 1, 1)]            # group 0 has no requirement: it may be split
    assert gr.runs_of([1, 1, 0, 0], [2, 2]) == [(0, 1, 1), (2, 3, 0)]
    with pytest.raises(gr.RunError):
        gr.runs_of([0, 1, 0], [1, 1])                               # group 0 twice
    with pytest.raises(gr.RunError):
        gr.runs_of([0, -1, 0], [1])                                 # an ungrouped preemptor in between


def test_a_gang_split_by_priorities_is_refused_by_both():
    sc = gs.gang_scene(7400, n=9, per_node=(2, 9), S=0, q=12, groups=3)
    grp = np.asarray(sc["pods"].group)[sc["pod_index"]]
    g = int(grp[grp >= 0][0])
    m = np.nonzero(grp == g)[0]
    other = np.nonzero(grp != g)[0]
    assert m.size >= 2 and other.size
    sc["priority"][m[0]] = 9000
    sc["priority"][other[0]] = 8000
    sc["priority"][m[1:]] = 7000
    sc["need"][:] = 0
    sc["need"][g] = 1
    with pytest.raises(gr.RunError):
        gs.expect_obj(sc, 4)
    with pytest.raises(gr.RunError):
        gs.expect(sc, 4)


def test_gang_order_and_gang_need_of_the_binding():
    capi = importlib.import_module("batch-scheduler_amd").capi
    rng = np.random.default_rng(5)
    for _ in range(50):
        q = int(rng.integers(1, 40))
        grp = rng.integers(-2, 4, size=q)
        pri = rng.choice([1, 5, 9], size=q)
        o = capi.gang_order(grp, pri)
        assert sorted(o.tolist()) == list(range(q))
        assert np.array_equal(o, gr.gang_order(grp, pri))
        p2, g2 = pri[o], grp[o]
        assert np.all(np.diff(p2) <= 0)
        assert np.array_equal(pc.slot_order(p2), np.arange(q))      # already in slot order: the stable sort keeps it
        for level in np.unique(pri):                                 # every gang of equal-priority members is one run
            seg = g2[p2 == level]
            for g in np.unique(seg[seg >= 0]):
                at = np.nonzero(seg == g)[0]
                assert at[-1] - at[0] + 1 == at.size
        # equal priorities, one group each: the caller's order
        assert np.array_equal(capi.gang_order(np.full(q, -1), np.zeros(q)), np.arange(q))
    assert capi.gang_order([1, 0, 1, -1, 0], [5, 5, 5, 5, 9]).tolist() == [4, 0, 2, 1, 3]

    class G:
        min_member = np.array([4, 2, 1, 3], np.uint32)
        status_scheduled = np.array([1, 2, 5, 0], np.uint32)
    assert capi.gang_need(G).tolist() == [3, 0, 0, 3]
    assert capi.gang_need(G, [2, 0, 0, 3]).tolist() == [1, 0, 0, 0]
    assert capi.gang_need(G).dtype == np.uint32


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_run_arrays_under_sanitizers(tmp_path):
    """csrc/bs_preempt_gang_runs.hpp compiled alone with tests/native/gang_runs_main.cpp under ASan + UBSan, against runs_of"""
    exe = str(tmp_path / "gang_runs")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "gang_runs_main.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(11)
    cases, lines = [], []
    for _ in range(300):
        q, g = int(rng.integers(0, 14)), int(rng.integers(0, 5))
        grp = np.sort(rng.integers(-2, g + 1, size=q)) if rng.random() < 0.6 else rng.integers(-2, g + 1, size=q)
        need = rng.integers(0, 3, size=g)
        cases.append((grp, need))
        lines.append(" ".join(map(str, [q, g, *grp.tolist(), *need.tolist()])))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    bad = 0
    for (grp, need), line in zip(cases, out):
        v = [int(x) for x in line.split()]
        q = len(grp)
        try:
            runs = gr.runs_of(grp, need)
        except gr.RunError:
            assert v[0] >= 0 and need[v[0]] > 0, line
            bad += 1
            continue
        assert v[0] == -1, line
        s_need, s_rlen = np.zeros(q, np.int64), np.zeros(q, np.int64)
        for s, e, g in runs:
            s_need[s:e + 1] = need[g]
            s_rlen[e] = e - s + 1
        assert v[1:1 + q] == s_need.tolist() and v[1 + q:] == s_rlen.tolist(), (grp, need, line)
    assert 10 < bad < len(cases) - 10


def test_the_gang_kernels_use_no_scratch():
    """k_gang_resolve<S>, S = 0..12: no scratch, and the workgroup sizes of pc_threads<S>() (256 threads at 12 scalar lanes)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    res = {k: v for k, v in kernel_resources.resources().items() if "k_gang_resolve" in k}
    assert len(res) == 13, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
