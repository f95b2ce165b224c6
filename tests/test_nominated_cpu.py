"""CPU tests of the resident nominated-pod table and of rule N (include/bsched.h; csrc/bs_nominated.hpp, bs_nominated_check.hpp): the table
model against an object-by-object rebuild, the two statements of rule N of tests/nominated_ref.py against each other and — with an empty
table — against the existing references, the hand known answers (tests/golden/nominated_hand_kats.json), the host-side argument checks
alone under the sanitizers, and where the new code sits in the build.  No GPU: nothing here creates a context."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import nominated_ref as nr
import preempt_gang_ref as gr
import preempt_gang_scenes as gs
import preempt_pdb_ref as pp
from preempt_scenes import kat_scene

bsa = importlib.import_module("batch-scheduler_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAP = 6
STATE = ("req", "pres", "bound_id", "bound_node")


def kats():
    with open(os.path.join(HERE, "golden", "nominated_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_rows(sc: dict):
    r, S = sc["rows"], sc["S"]
    t = nr.NomTable(S)
    t.load(len(sc["nodes"]["flags"]), r["node"], r["priority"], np.array(r["req"], np.int64).reshape(4 + S, -1), r["pres"])
    return t


# ---- the table model ---------------------------------------------------------------------------------------------------------------
def _table_history(seed: int):
    """a seeded history of accepted and refused calls on one table: (model, accepted history, pods, refusals seen)"""
    rng = np.random.default_rng(seed)
    S = int(rng.integers(0, 3))
    sc, _ = pp.pdb_scene(seed, n=6, per_node=(1, 3), S=S, q=4, groups=2, share=0.0)
    pods, n = sc["pods"], sc["nodes"].n
    t = nr.NomTable(S)
    hist, refused = [], set()
    m = int(rng.integers(0, 6))
    load = ("load", rng.integers(0, n, size=m).astype(np.uint32), rng.integers(-5, 50, size=m).astype(np.int32),
            rng.integers(0, 1000, size=(4 + S, m)).astype(np.int64), rng.integers(0, 8, size=m).astype(np.uint32))
    t.load(n, *load[1:])
    hist.append(load)
    for _ in range(int(rng.integers(2, 7))):
        live = t.id.copy()
        k = int(rng.integers(0, live.size + 1))
        remove = rng.permutation(live)[:k].astype(np.uint32)
        ni = int(rng.integers(0, 4))
        pod_index = rng.integers(0, pods.p, size=ni).astype(np.uint32)
        node = rng.integers(0, n, size=ni).astype(np.uint32)
        prio = rng.integers(-5, 50, size=ni).astype(np.int32)
        bad = int(rng.integers(0, 8))
        if bad == 0:
            remove = np.append(remove, np.uint32(t.ids + 3))                                   # unknown
        elif bad == 1 and remove.size:
            remove = np.append(remove, remove[0])                                              # repeated
        elif bad == 2 and t.ids > live.size:
            remove = np.append(remove, np.setdiff1d(np.arange(t.ids, dtype=np.uint32), live)[:1])   # dead
        elif bad == 3 and ni:
            node[0] = n                                                                        # node >= n
        elif bad == 4 and ni:
            pod_index[0] = pods.p                                                              # pod_index >= p
        before = t.read()
        try:
            t.apply(remove, pod_index, node, prio, pods)
            hist.append(("apply", remove, pod_index, node, prio))
        except nr.NomRefused as e:
            refused.add(str(e).split(":")[1].strip())
            after = t.read()
            assert all(np.array_equal(before[f], after[f]) for f in before), "a refused call changed the model"
    return t, hist, pods, S, refused


def test_the_table_model_against_the_object_rebuild_over_seeded_scenes():
    seen = set()
    for seed in range(200):
        t, hist, pods, S, refused = _table_history(seed)
        seen |= refused
        got, exp = t.read(), nr.objects_as_rows(nr.rebuild_rows(S, hist, pods), S)
        for f in got:
            assert np.array_equal(got[f], exp[f]), f"seed {seed}: {f}: {got[f].tolist()} vs {exp[f].tolist()}"
        assert np.all(np.diff(got["id"].astype(np.int64)) > 0), "rows are in ascending id"
        assert t.ids == hist[0][1].size + sum(len(h[2]) for h in hist[1:]), "ids are never reused before the next load"
    assert {"unknown id", "repeated id", "dead id", "pod index or node"} <= seen, seen


def test_the_model_limits():
    sc, _ = pp.pdb_scene(3, n=4, per_node=(1, 2), S=0, q=2, groups=0, share=0.0)
    t = nr.NomTable(0)
    with pytest.raises(nr.NomRefused, match="BS_ERR_STATE"):
        t.apply([], [], [], [], sc["pods"])
    with pytest.raises(nr.NomRefused, match="BS_ERR_CAPACITY"):
        t.load(4, [], [], np.zeros((4, 0)), [], m=nr.NOM_MAX + 1)
    t.load(4, [0, 1], [1, 2], np.zeros((4, 2)), [0, 0])
    with pytest.raises(nr.NomRefused, match="BS_ERR_CAPACITY"):
        t.apply([], [0, 1], [0, 0], [1, 1], sc["pods"], max_rows=3)
    with pytest.raises(nr.NomRefused, match="BS_ERR_CAPACITY"):
        t.apply([0], [0, 1], [0, 0], [1, 1], sc["pods"], max_ids=3)
    assert t.apply([0], [0], [0], [1], sc["pods"], max_rows=2, max_ids=3) == 2           # exactly the limits is fine
    with pytest.raises(nr.NomRefused, match="BS_ERR_STATE"):
        t.apply([], [], [], [], sc["pods"], n_now=5)
    with pytest.raises(nr.NomRefused, match="BS_ERR_INVALID"):
        t.load(4, [4], [1], np.zeros((4, 1)), [0])


# ---- rule N: the two statements ------------------------------------------------------------------------------------------------------
def _scene(seed: int, gang: bool):
    S = seed % 3
    if gang:
        sc = gs.gang_scene(seed, n=6, per_node=(2, 6), S=S, q=10, groups=4, share=0.2)
    else:
        sc, bits = pp.pdb_scene(seed, n=6, per_node=(2, 6), S=S, q=8, groups=3, share=0.2)
        sc["violating"] = bits
    return sc


def _args(sc):
    return sc["nodes"], sc["fit"], sc["pods"], sc["bound"], sc["S"], sc["pod_index"], sc["priority"], sc["protected"]


def _prep(sc):
    return pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], sc["violating"])


def _same_res(a, b, where):
    for f in pp.FIELDS:
        assert np.array_equal(a[f], b[f]), f"{where}: {f}: {a[f].tolist()} vs {b[f].tolist()}"


def _same_plan(a, b, where, gang=False):
    _same_res(a["res"], b["res"], where)
    for f in STATE + (("slot_voided", "group_placed") if gang else ()):
        assert np.array_equal(a[f], b[f]), f"{where}: {f}"


def _three(sc, rows, apply, assume):
    """(run, commit, gang or None) by the object statement and by the array statement"""
    n, fit, pods, bound, S, pi, pr_, prot = _args(sc)
    prep, bits = _prep(sc), sc["violating"]
    obj = [nr.run_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, bits, rows),
           nr.plan_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, bits, rows, None, apply, assume)]
    arr = [nr.run_nom_np(prep, fit, pods, pi, pr_, prot, CAP, rows),
           nr.commit_nom_np(prep, fit, pods, bound, pi, pr_, prot, CAP, rows, apply, assume)]
    if "need" in sc:
        obj.append(nr.plan_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, bits, rows, sc["need"], apply, assume))
        arr.append(nr.gang_nom_np(prep, fit, pods, bound, pi, pr_, prot, sc["need"], CAP, rows, apply, assume))
    return obj, arr


def test_the_two_statements_agree_and_the_table_matters():
    """300 scenes, 100 each with the focus on run, commit and gang (every scene runs run and commit; the gang scenes all three).  The
    condition that keeps the comparison from proving little: in at least a third of the scenes the table changes a node, a victim list
    or a pick key — counted on the model alone, per call."""
    hit = {"run": 0, "commit": 0, "gang": 0}
    total = {"run": 0, "commit": 0, "gang": 0}
    for seed in range(300):
        gang = seed >= 200
        sc = _scene(1000 + seed, gang)
        rows = nr.nom_rows_for(sc, seed)
        apply, assume = bool(seed & 1), bool(seed & 2) and bool(seed & 1)
        obj, arr = _three(sc, rows, apply, assume)
        _same_res(obj[0], arr[0], f"seed {seed} run")
        _same_plan(obj[1], arr[1], f"seed {seed} commit")
        if gang:
            _same_plan(obj[2], arr[2], f"seed {seed} gang", gang=True)
        bare, _ = _three(sc, None, apply, assume)
        for name, i in (("run", 0), ("commit", 1)) + ((("gang", 2),) if gang else ()):
            a, b = (obj[i], bare[i]) if i == 0 else (obj[i]["res"], bare[i]["res"])
            total[name] += 1
            hit[name] += nr.changed(a, b)
    for name in hit:
        assert 3 * hit[name] >= total[name], f"the table changes {name}'s answer in {hit[name]} of {total[name]} scenes only"


def test_an_empty_table_is_the_existing_references_and_pins_the_restated_loops():
    """no table, and a loaded table without rows: both statements equal preempt_pdb_obj / commit_pdb_obj / gang_obj and their numpy
    twins over the existing scene generators — which also pins the slot loops nominated_ref restates"""
    for seed in range(40):
        gang = seed >= 20
        sc = _scene(seed, gang)
        n, fit, pods, bound, S, pi, pr_, prot = _args(sc)
        bits, prep = sc["violating"], _prep(sc)
        empty = nr.NomTable(S)
        empty.load(n.n, [], [], np.zeros((4 + S, 0)), [])
        for rows in (None, empty.read()):
            for apply, assume in ((False, False), (True, False), (True, True)):
                obj, arr = _three(sc, rows, apply, assume)
                w = f"seed {seed} apply={apply} assume={assume}"
                _same_res(obj[0], pp.preempt_pdb_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, bits), w + " run obj")
                _same_res(arr[0], pp.preempt_pdb_np(prep, fit, pods, pi, pr_, prot, CAP), w + " run np")
                _same_plan(obj[1], pp.commit_pdb_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, bits, apply, assume), w + " commit obj")
                _same_plan(arr[1], pp.commit_pdb_np(prep, fit, pods, bound, pi, pr_, prot, CAP, apply, assume), w + " commit np")
                if gang:
                    _same_plan(obj[2], gr.gang_obj(n, fit, pods, bound, S, pi, pr_, prot, sc["need"], CAP, apply, assume, bits), w + " gang obj", True)
                    _same_plan(arr[2], gr.gang_np(prep, fit, pods, bound, pi, pr_, prot, sc["need"], CAP, apply, assume), w + " gang np", True)


def test_apply_and_assume_leave_node_requests_as_without_a_table():
    """invariant 1: the rows' sum is never stored.  Where the table changes no answer, the state APPLY / ASSUME leave is the state
    without a table; where it does, the state differs by victims and nominees only — never by a row"""
    for seed in range(30):
        sc = _scene(2000 + seed, False)
        n, fit, pods, bound, S, pi, pr_, prot = _args(sc)
        rows = nr.nom_rows_for(sc, seed)
        got = nr.plan_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, sc["violating"], rows, None, True, True)
        # replay the answers on a bare state: victims leave, nominees arrive, nothing else
        req = np.array(n.requested, np.int64, copy=True)
        L = 4 + S
        with np.errstate(over="ignore"):
            for i in range(len(pi)):
                k = int(got["res"]["node"][i])
                if k < 0:
                    continue
                for v in got["res"]["victims"][i, : int(got["res"]["n_victims"][i])]:
                    stored, _ = nr._stored(bound.req[:L, [int(v)]], bound.req_present[[int(v)]], S)
                    req[:, k] -= stored[:, 0]
                stored, _ = nr._stored(pods.req[:L, [int(pi[i])]], pods.req_present[[int(pi[i])]], S)
                req[:, k] += stored[:, 0]
        eff = lambda r, p: np.array([[r[l, k] if l < 4 or (int(p[k]) >> (l - 4)) & 1 else 0 for k in range(n.n)] for l in range(L)])
        assert int(got["res"]["n_victims"].max(initial=0)) <= CAP, "the replay needs every victim listed"
        assert np.array_equal(eff(got["req"], got["pres"]), eff(req, got["pres"])), f"seed {seed}"


# ---- the hand known answers ----------------------------------------------------------------------------------------------------------
def _check_expect(res, expect, where):
    for i, e in enumerate(expect):
        assert int(res["node"][i]) == e["node"], f"{where}: preemptor {i}: node {res['node'][i]}"
        assert int(res["n_candidates"][i]) == e["n_candidates"], f"{where}: preemptor {i}: n_candidates {res['n_candidates'][i]}"
        nv = int(res["n_victims"][i])
        assert res["victims"][i, :nv].tolist() == e["victims"], f"{where}: preemptor {i}: victims {res['victims'][i, :nv].tolist()}"


@pytest.mark.parametrize("sc", kats(), ids=lambda s: s["name"])
def test_hand_known_answers(sc):
    assert sc["cite"]
    s = kat_scene(sc)
    n, fit, pods, bound, S, pi, pr_, prot = _args(s)
    table = kat_rows(sc)
    prep = pp.PdbPrep(n, bound, S, None)
    if sc["call"] == "run":
        _check_expect(nr.run_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, None, table.read()), sc["expect"], "obj")
        _check_expect(nr.run_nom_np(prep, fit, pods, pi, pr_, prot, CAP, table.read()), sc["expect"], "np")
    elif sc["call"] == "gang":
        got = nr.plan_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, None, table.read(), sc["need"], True, False)
        _check_expect(got["res"], sc["expect"], "obj")
        _check_expect(nr.gang_nom_np(prep, fit, pods, bound, pi, pr_, prot, sc["need"], CAP, table.read(), True, False)["res"], sc["expect"], "np")
        assert got["slot_voided"].tolist() == sc["expect_voided"]
        ids = nr.nominate_rows(table, got["res"], pi, pr_, pods)
        assert table.read()["id"].size == sc["expect_rows"] and np.all(ids == nr.NONE)
    else:
        second = sc["second"]
        for flag in ("nominate", "assume"):
            t = kat_rows(sc)
            first = nr.plan_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, None, t.read(), None, True, flag == "assume")
            _check_expect(first["res"], sc["expect_first"], flag + " first")
            if flag == "nominate":
                assert nr.nominate_rows(t, first["res"], pi, pr_, pods).tolist() == [0]
            nodes2 = bsa.soa.Nodes(n.allocatable, first["req"], n.allocatable_present, first["pres"], n.flags)
            keep = np.isin(np.arange(bound.b), first["bound_id"])
            assert keep.all(), "the first call of these vectors evicts nobody"
            got = nr.run_nom_obj(nodes2, fit, pods, bound, S, second["pod_index"], second["priority"], prot, CAP, None, t.read())
            _check_expect(got, sc["expect_" + flag], flag + " second")


def test_the_hand_vectors_cover_the_issue_list():
    names = [s["name"] for s in kats()]
    assert 8 <= len(names) <= 10 and len(set(names)) == len(names)
    assert "D5." in open(os.path.join(ROOT, "include", "bsched.h")).read()


# ---- the host-side argument checks, alone, under sanitizers ----------------------------------------------------------------------------
OK, NULL, NODE, UNKNOWN, DEAD, TWICE, PODIDX, ROWS, IDSPACE = range(9)


def test_argument_checks_under_sanitizers(tmp_path):
    """csrc/bs_nominated_check.hpp compiled alone with tests/native/nominated_check_main.cpp under ASan + UBSan: every refusal, the id-space
    and BS_NOM_MAX edges, NULL with count 0"""
    exe = str(tmp_path / "nominated_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "nominated_check_main.cpp"), "-o", exe], check=True)
    M, I = 1 << 16, 1 << 24
    lst = lambda v: " ".join(str(x) for x in v)
    cases = [
        (f"D 4 0 1 {M}", OK),                                           # NULL with count 0
        (f"D 4 3 0 {M} 0 3 1", OK),
        (f"D 4 3 0 {M} 0 4 1", NODE),
        (f"D 4 3 1 {M} 0 1 2", NULL),
        (f"D 4 {M} 0 {M} " + lst([i % 4 for i in range(M)]), OK),       # exactly BS_NOM_MAX
        (f"D 4 {M + 1} 0 {M}", ROWS),                                   # one more: refused before the list is walked
        (f"D 0 1 0 {M} 0", NODE),                                       # no nodes at all
        (f"A 0 0  0 1  0 1    5 4 {M} {I}", OK),                        # both counts 0, NULL lists
        (f"A 3 5 0 2 4  2 0 4 0  1 0 1 2  5 4 {M} {I}", OK),
        (f"A 3 5 0 2 4  1 1    0 1    5 4 {M} {I}", NULL),              # remove NULL with a count
        (f"A 3 5 0 2 4  0 1    1 1    5 4 {M} {I}", NULL),              # insert NULL with a count
        (f"A 3 5 0 2 4  1 0 5  0 1    5 4 {M} {I}", UNKNOWN),           # id == ids
        (f"A 3 5 0 2 4  1 0 3  0 1    5 4 {M} {I}", DEAD),              # inside the id space, not live
        (f"A 3 5 0 2 4  2 0 2 2  0 1  5 4 {M} {I}", TWICE),
        (f"A 0 5   1 0 3  0 1    5 4 {M} {I}", DEAD),                   # an empty table with an id space
        (f"A 3 5 0 2 4  0 1  1 0 5 0  5 4 {M} {I}", PODIDX),            # pod_index == p
        (f"A 3 5 0 2 4  0 1  1 0 4 4  5 4 {M} {I}", NODE),              # node == n
        (f"A 3 5 0 2 4  0 1  1 0 1 2  5 4 3 {I}", ROWS),                # 3 live + 1 over a limit of 3
        (f"A 3 5 0 2 4  1 0 2  1 0 1 2  5 4 3 {I}", OK),                # ... one leaves first: exactly the limit
        (f"A 3 5 0 2 4  0 1  1 0 1 2  5 4 {M} 5", IDSPACE),             # ids 5 + 1 over an id space of 5
        (f"A 3 5 0 2 4  0 1  1 0 1 2  5 4 {M} 6", OK),                  # exactly the id space
        (f"A 3 {I - 1} 0 2 4  0 1  2 0 1 1 2 2  5 4 {M} {I}", IDSPACE),  # the real edge: 2^24 - 1 + 2
        (f"A 3 {I - 1} 0 2 4  0 1  1 0 1 2  5 4 {M} {I}", OK),
        (f"N {M - 2} 10 2 {M} {I}", OK),
        (f"N {M - 2} 10 3 {M} {I}", ROWS),
        (f"N 5 {I - 4} 4 {M} {I}", OK),
        (f"N 5 {I - 4} 5 {M} {I}", IDSPACE),
        (f"N 5 10 4294967295 {M} {I}", ROWS),                           # the sum is taken in 64 bits
    ]
    out = subprocess.run([exe], input="\n".join(c for c, _ in cases) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert out[-1] == "ok"
    assert [int(x) for x in out[:-1]] == [e for _, e in cases], list(zip([c[:40] for c, _ in cases], out))


# ---- where the new code sits -----------------------------------------------------------------------------------------------------------
def test_the_new_headers_are_listed_with_the_unit_that_includes_them():
    build = bsa.build
    assert {"bs_nominated.hpp", "bs_nominated_check.hpp"} <= set(build.UNITS["tu_nominated.hip"])
    src = open(os.path.join(ROOT, "batch-scheduler_amd", "csrc", "tu_nominated.hip")).read()
    assert '#include "bs_nominated.hpp"' in src and '#include "bs_nominated_check.hpp"' in src
    check = open(os.path.join(ROOT, "batch-scheduler_amd", "csrc", "bs_nominated_check.hpp")).read()
    assert "hip" not in check.split("#pragma once")[1].lower(), "the check header is plain C++"
    assert "bs_nominated.hpp" not in build.UNITS["tu_preempt.hip"], "the preemption calls reach the table through bs_ctx.hpp's declarations only"
    for other in ("tu_preempt.hip", "tu_bound.hip", "tu_bind.hip", "tu_wait.hip", "bsched.hip"):
        assert "bs_nominated.hpp" not in open(os.path.join(ROOT, "batch-scheduler_amd", "csrc", other)).read(), "the k_nm_* kernels are emitted by one unit"


# waves per SIMD (512 registers a lane, allocated in eights) of every touched kernel on the commit before the table, S = 0..12; the
# kernels with the nominee walk must not fall below them (measured with tools/kernel_resources.py on that build)
WAVES_BEFORE = {
    "k_preempt_scan": (8, 8, 8, 7, 6, 5, 5, 5, 4, 4, 4, 4, 4),
    "k_preempt_pick": (8, 8, 7, 6, 5, 5, 4, 4, 3, 3, 3, 3, 2),
    "k_pc_scan": (4, 4, 4, 4, 4, 3, 3, 3, 3, 3, 3, 2, 2),
    "k_pc_resolve": (4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2),
    "k_gang_resolve": (4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2),
}


def test_touched_and_new_kernels_use_no_scratch_and_lose_no_wave():
    import re
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources()
    seen = {}
    for name, v in all_k.items():
        m = re.match(r"_ZN2bs\d+(k_\w+?)(?:ILi(\d+)E|E)", name)
        if not m or not (m.group(1) in WAVES_BEFORE or m.group(1).startswith("k_nm_")):
            continue
        assert v["scratch"] == 0, (name, v)
        if m.group(1) in WAVES_BEFORE:
            S = int(m.group(2))
            waves = min(8, 512 // ((max(v["vgpr"], 1) + 7) // 8 * 8))
            assert waves >= WAVES_BEFORE[m.group(1)][S], f"{m.group(1)}<{S}>: {v['vgpr']} VGPRs = {waves} waves, {WAVES_BEFORE[m.group(1)][S]} before"
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
    assert {k: seen.get(k) for k in WAVES_BEFORE} == {k: 13 for k in WAVES_BEFORE}, seen
    assert (seen.get("k_nm_mark"), seen.get("k_nm_chains"), seen.get("k_nm_move"), seen.get("k_nm_gather")) == (1, 1, 13, 13), seen
    units = {v["unit"] for k, v in all_k.items() if "k_nm_" in k}
    assert len(units) == 1, "the k_nm_* kernels are emitted by one unit"
