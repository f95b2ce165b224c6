"""CPU tests of BS_PREEMPT_CLEAR_LOWER (include/bsched.h, rule C; csrc/bs_preempt_clear.hpp, bs_preempt_clear_list.hpp): the two statements of
tests/preempt_clear_ref.py against each other over seeded scenes in every flag mode, against nominated_ref where nothing can be cleared,
against the call taken apart into single-slot calls, the hand known answers (tests/golden/preempt_clear_hand_kats.json), the host-side list
logic alone under the sanitizers, the ABI, and where the new code sits in the build.  No GPU: nothing here creates a context."""
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nominated_ref as nr
import preempt_clear_ref as cr
import preempt_commit_ref as pc
import preempt_pdb_ref as pp
from preempt_scenes import kat_scene

bsa = importlib.import_module("batch-scheduler_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAP = 6
STATE = ("req", "pres", "bound_id", "bound_node")
MODES = ("plan", "apply", "assume", "nominate")          # flags 0, APPLY, APPLY|ASSUME, APPLY|NOMINATE — each with CLEAR_LOWER


def kats():
    with open(os.path.join(HERE, "golden", "preempt_clear_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_rows(sc: dict):
    r, S = sc["rows"], sc["S"]
    t = nr.NomTable(S)
    t.load(len(sc["nodes"]["flags"]), r["node"], r["priority"], np.array(r["req"], np.int64).reshape(4 + S, -1), r["pres"])
    return t


def _args(sc):
    return sc["nodes"], sc["fit"], sc["pods"], sc["bound"], sc["S"], sc["pod_index"], sc["priority"], sc["protected"]


def _prep(sc):
    return pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], sc["violating"])


def _np_args(sc):
    return _prep(sc), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"], sc["protected"]


def _same_res(a, b, where):
    for f in pp.FIELDS:
        assert np.array_equal(a[f], b[f]), f"{where}: {f}: {a[f].tolist()} vs {b[f].tolist()}"


def _same_plan(a, b, where, gang=False, cleared=True):
    _same_res(a["res"], b["res"], where)
    for f in STATE + (("slot_voided", "group_placed") if gang else ()):
        assert np.array_equal(a[f], b[f]), f"{where}: {f}"
    if cleared:
        for f in cr.CLEARED:
            assert np.array_equal(a["cleared"][f], b["cleared"][f]), f"{where}: cleared {f}: {a['cleared'][f].tolist()} vs {b['cleared'][f].tolist()}"


def _both(sc, rows, mode):
    """the scene's call (gang where the scene has needs) by the object statement and by the threshold statement"""
    apply, assume = mode != "plan", mode == "assume"
    n, fit, pods, bound, S, pi, pr_, prot = _args(sc)
    need = sc.get("need")
    obj = cr.plan_clear_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, sc["violating"], rows, need, apply, assume)
    if need is None:
        arr = cr.commit_clear_np(*_np_args(sc), CAP, rows, apply, assume)
    else:
        arr = cr.gang_clear_np(*_np_args(sc), need, CAP, rows, apply, assume)
    return obj, arr


def _table(sc, rows):
    t = nr.NomTable(sc["S"])
    t.load(sc["nodes"].n, rows["node"], rows["priority"], rows["req"], rows["req_present"])
    return t


def _plan_differs(a, b):
    return not np.array_equal(a["node"], b["node"]) or not np.array_equal(a["victims"], b["victims"]) or not np.array_equal(a["n_victims"], b["n_victims"])


# ---- the two statements ----------------------------------------------------------------------------------------------------------------
def test_the_two_statements_agree_in_every_flag_mode_and_the_flag_matters():
    """100 commit scenes and 200 gang scenes, the flag mode by seed.  The conditions that keep the comparison from proving little, counted
    on the models alone: the flagged plan differs from the flag-less one (nominated_ref) in a node or a victim list in at least a quarter
    of the scenes of each call, and at least 20 gang scenes void a run that had cleared a row."""
    differs, total, void_cleared, some_cleared = {False: 0, True: 0}, {False: 0, True: 0}, 0, 0
    seen_modes = {False: set(), True: set()}
    for seed in range(300):
        gang = seed >= 100
        sc = cr.clear_scene(5000 + seed, gang, n=8, q=14)
        rows = cr.clear_rows_for(sc, seed, density=1.0, per_node=(2, 4), heavy=0.5)
        mode = MODES[seed % 4]
        seen_modes[gang].add(mode)
        obj, arr = _both(sc, rows, mode)
        _same_plan(obj, arr, f"seed {seed} {mode}", gang=gang)
        ta, tb = _table(sc, rows), _table(sc, rows)
        ia = cr.table_after(ta, obj, sc["pod_index"], sc["priority"], sc["pods"], mode != "plan", mode == "nominate")
        ib = cr.table_after(tb, arr, sc["pod_index"], sc["priority"], sc["pods"], mode != "plan", mode == "nominate")
        assert np.array_equal(ia, ib) and all(np.array_equal(ta.read()[f], tb.read()[f]) for f in ta.read()), f"seed {seed}: the table afterwards"
        assert not np.isin(arr["cleared"]["id"], ta.read()["id"]).any() or mode == "plan", "a cleared id is dead after APPLY"
        apply, assume = mode != "plan", mode == "assume"
        if gang:
            bare = nr.gang_nom_np(*_np_args(sc), sc["need"], CAP, rows, apply, assume)
            void_cleared += cr.voided_a_clearing(*_np_args(sc), sc["need"], CAP, rows)
        else:
            bare = nr.commit_nom_np(*_np_args(sc), CAP, rows, apply, assume)
        total[gang] += 1
        differs[gang] += _plan_differs(arr["res"], bare["res"])
        some_cleared += arr["cleared"]["id"].size > 0
    assert seen_modes[False] == seen_modes[True] == set(MODES)
    print(f"flagged plan differs: commit {differs[False]}/{total[False]}, gang {differs[True]}/{total[True]}; gang scenes voiding a clearing run: "
          f"{void_cleared}; scenes with a cleared row: {some_cleared}")
    for gang in (False, True):
        assert 4 * differs[gang] >= total[gang], f"the flag changes the plan in {differs[gang]} of {total[gang]} scenes only (gang={gang})"
    assert void_cleared >= 20, f"{void_cleared} gang scenes void a run that had cleared something"


def test_with_no_row_below_any_preemptor_the_plan_is_nominated_refs():
    """rows at or above the highest preemptor priority can never be cleared: both statements equal nominated_ref's plans field for field
    (which also pins the slot loops preempt_clear_ref restates), and the report is empty; so do no table and an empty table"""
    for seed in range(40):
        gang = seed >= 20
        sc = cr.clear_scene(7000 + seed, gang, n=6, q=10)
        rows = cr.clear_rows_for(sc, seed)
        top = int(np.max(sc["priority"]))
        rows["priority"] = np.maximum(rows["priority"], top + (seed & 1)).astype(np.int32)      # equal to the top preemptor's counts as "not below"
        empty = nr.NomTable(sc["S"])
        empty.load(sc["nodes"].n, [], [], np.zeros((4 + sc["S"], 0)), [])
        n, fit, pods, bound, S, pi, pr_, prot = _args(sc)
        for r in (rows, None, empty.read()):
            for mode in MODES[:3]:
                apply, assume = mode != "plan", mode == "assume"
                obj, arr = _both(sc, r, mode)
                w = f"seed {seed} {mode}"
                exp_obj = nr.plan_nom_obj(n, fit, pods, bound, S, pi, pr_, prot, CAP, sc["violating"], r, sc.get("need"), apply, assume)
                exp_arr = (nr.gang_nom_np(*_np_args(sc), sc["need"], CAP, r, apply, assume) if gang else
                           nr.commit_nom_np(*_np_args(sc), CAP, r, apply, assume))
                _same_plan(obj, exp_obj, w + " obj", gang=gang, cleared=False)
                _same_plan(arr, exp_arr, w + " np", gang=gang, cleared=False)
                assert obj["cleared"]["id"].size == 0 and arr["cleared"]["id"].size == 0


def test_one_flagged_call_equals_single_slot_calls_with_a_plain_removal_in_between():
    """bs_preempt_commit(APPLY | NOMINATE | CLEAR_LOWER) of q slots, preemptors passed in slot order, against q flag-less single-slot
    calls (nominated_ref.commit_nom_np, APPLY | NOMINATE) with NomTable.apply removing the lower rows on the taken node in between:
    the answers (n_candidates included), the node requests, the bound table, the table and the report"""
    cleared_rows = 0
    for seed in range(60):
        sc = cr.clear_scene(9000 + seed, False, n=6, q=8)
        o = pc.slot_order(sc["priority"])
        sc["pod_index"], sc["priority"] = sc["pod_index"][o], sc["priority"][o]
        rows = cr.clear_rows_for(sc, seed, density=1.0, per_node=(1, 3))
        n, fit, pods, bound, S, pi, pr_, prot = _args(sc)
        one = cr.commit_clear_np(*_np_args(sc), CAP, rows, True, False)
        t1 = _table(sc, rows)
        cr.table_after(t1, one, pi, pr_, pods, True, True)
        t2 = _table(sc, rows)
        seq = cr.one_by_one(n, fit, pods, bound, S, pi, pr_, prot, CAP, sc["violating"], t2)
        _same_res(one["res"], seq["res"], f"seed {seed}")
        eff = lambda r, p: np.array([[r[l, k] if l < 4 or (int(p[k]) >> (l - 4)) & 1 else 0 for k in range(n.n)] for l in range(4 + S)])
        assert np.array_equal(eff(one["req"], one["pres"]), eff(seq["req"], seq["pres"])), f"seed {seed}: node requests"
        assert np.array_equal(np.sort(one["bound_id"]), seq["bound_id"]), f"seed {seed}: bound table"
        for f in cr.CLEARED:
            assert np.array_equal(one["cleared"][f], seq["cleared"][f]), f"seed {seed}: cleared {f}"
        a, b = t1.read(), t2.read()
        # the single calls append a nominee and remove rows in turns, the one call removes first: the same rows, as sets by id
        for f in ("node", "priority", "req_present"):
            assert np.array_equal(a[f][np.argsort(a["id"])], b[f][np.argsort(b["id"])]) and np.array_equal(np.sort(a["id"]), np.sort(b["id"])), f"seed {seed}: table {f}"
        cleared_rows += one["cleared"]["id"].size
    assert cleared_rows >= 60, cleared_rows


# ---- the hand known answers ----------------------------------------------------------------------------------------------------------
def _check_expect(res, expect, where):
    for i, e in enumerate(expect):
        assert int(res["node"][i]) == e["node"], f"{where}: preemptor {i}: node {res['node'][i]}"
        assert int(res["n_candidates"][i]) == e["n_candidates"], f"{where}: preemptor {i}: n_candidates {res['n_candidates'][i]}"
        nv = int(res["n_victims"][i])
        assert res["victims"][i, :nv].tolist() == e["victims"], f"{where}: preemptor {i}: victims {res['victims'][i, :nv].tolist()}"


def check_kat(got: dict, table_ids, sc: dict, where: str):
    """shared with the GPU test: a plan dict (res, cleared, and slot_voided / group_placed for a gang call) against the vector"""
    _check_expect(got["res"], sc["expect"], where)
    rows = [[int(got["cleared"][f][j]) for f in cr.CLEARED] for j in range(len(got["cleared"]["id"]))]
    assert rows == sc["expect_cleared"], f"{where}: cleared {rows}"
    assert [int(x) for x in table_ids] == sc["expect_table_ids"], f"{where}: table ids {list(table_ids)}"
    if sc["call"] == "gang":
        assert [int(x) for x in got["slot_voided"]] == sc["expect_voided"], where
        assert [int(x) for x in got["group_placed"]] == sc["expect_placed"], where


@pytest.mark.parametrize("sc", kats(), ids=lambda s: s["name"])
def test_hand_known_answers(sc):
    assert "rule C" in sc["cite"]
    s = kat_scene(sc)
    s["violating"] = None
    if sc["call"] == "gang":
        s["need"] = np.array(sc["need"], np.uint32)
    rows = kat_rows(sc).read()
    mode = sc["mode"]
    for name, got in zip(("obj", "np"), _both(s, rows, mode)):
        t = kat_rows(sc)
        cr.table_after(t, got, s["pod_index"], s["priority"], s["pods"], mode != "plan", mode == "nominate")
        check_kat(got, t.read()["id"], sc, name)
        if "expect_table" in sc:
            for f, v in sc["expect_table"].items():
                assert t.read()[f].tolist() == v, f"{name}: table {f}"
    if "expect_nodes_without_flag" in sc:
        bare = nr.commit_nom_np(pp.PdbPrep(s["nodes"], s["bound"], s["S"], None), s["fit"], s["pods"], s["bound"], s["pod_index"], s["priority"],
                                s["protected"], CAP, rows)
        assert bare["res"]["node"].tolist() == sc["expect_nodes_without_flag"]


def test_the_hand_vectors_cover_the_issue_list():
    names = [s["name"] for s in kats()]
    assert len(names) >= 8 and len(set(names)) == len(names)
    for must in ("a_later_slot_fits_only_because_an_earlier_slot_cleared_a_row", "an_equal_priority_row_is_not_cleared",
                 "a_row_on_another_node_is_untouched", "a_victim_free_take_still_clears", "a_voided_run_gives_its_rows_back",
                 "a_row_cleared_by_a_standing_slot_and_by_a_voided_run_stays_cleared", "the_by_column_with_two_takers_of_one_node",
                 "the_rows_nominate_appends_are_not_cleared"):
        assert must in names, must
    assert all(len(s["nodes"]["flags"]) <= 3 for s in kats())


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_the_flag_and_the_entry_point_are_in_the_header_and_the_abi_list():
    h = open(os.path.join(ROOT, "include", "bsched.h")).read()
    assert re.search(r"#define\s+BS_PREEMPT_CLEAR_LOWER\s+8u", h)
    assert re.search(r"int bs_preempt_cleared_read\(bs_ctx\* ctx, uint32_t cap, uint32_t\* id[^;]*uint32_t\* node[^;]*int32_t\* priority[^;]*uint32_t\* by[^;]*"
                     r"uint32_t\* n_out\);", h)
    assert re.search(r"#define\s+BS_ABI_VERSION\s+7u", h), "the change is additive"
    assert "rule C" in h
    assert "bs_preempt_cleared_read" in bsa.capi.ABI_SYMBOLS
    assert bsa.soa.PREEMPT_CLEAR_LOWER == 8
    assert not bsa.soa.PREEMPT_CLEAR_LOWER & (bsa.soa.PREEMPT_APPLY | bsa.soa.PREEMPT_ASSUME | bsa.soa.PREEMPT_NOMINATE)
    src = open(os.path.join(ROOT, "batch-scheduler_amd", "capi.py")).read()
    assert src.count("clear_lower: bool = False") == 2


# ---- the host-side list logic, alone, under sanitizers ---------------------------------------------------------------------------------
OK, NULL, STATE_, COUNT, ORDER, DEAD, NODE = range(7)


def test_list_logic_under_sanitizers(tmp_path):
    """csrc/bs_preempt_clear_list.hpp compiled alone with tests/native/preempt_clear_list_main.cpp under ASan + UBSan: the check of the
    device's list, and the read's NULL, state and cap rules with arrays of exactly cap entries"""
    exe = str(tmp_path / "preempt_clear_list")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "preempt_clear_list_main.cpp"), "-o", exe], check=True)
    cases = [
        ("C 3 2 5 9  4 2  0 0", "0"),                                   # nothing cleared, NULL columns
        ("C 3 2 5 9  4 2  2 0  2 9  0 3  1 0", "0"),
        ("C 3 2 5 9  4 2  3 0  2 5 9  0 3 1  1 0 1", "0"),               # the whole table
        ("C 3 2 5 9  4 2  4 1", str(COUNT)),                             # more rows than the table: judged before a column is read
        ("C 3 2 5 9  4 2  2 1", str(NULL)),
        ("C 3 2 5 9  4 2  2 0  9 2  0 3  1 0", str(ORDER)),
        ("C 3 2 5 9  4 2  2 0  2 2  0 3  1 0", str(ORDER)),              # twice
        ("C 3 2 5 9  4 2  1 0  4  0  1", str(DEAD)),
        ("C 3 2 5 9  4 2  1 0  5  4  1", str(NODE)),                     # node == n
        ("C 3 2 5 9  4 2  1 0  5  3  2", str(NODE)),                     # by == q
        ("C 0  4 2  0 1", "0"),                                          # an empty table
        ("C 0  4 2  1 0  0  0  0", str(COUNT)),
        ("R 0 0  0 1 0", f"{STATE_} 57005"),                             # no flagged call: n_out is not written
        ("R 1 0  0 1 0", "0 0"),                                         # a flagged call that cleared nothing, cap 0, NULL columns
        ("R 1 0  4 0 0", "0 0"),
        ("R 1 3  2 5 9  0 3 1  7 -2 8  1 0 1  0 1 0", "0 3"),            # cap 0: the count alone
        ("R 1 3  2 5 9  0 3 1  7 -2 8  1 0 1  2 0 0", "0 3 2 5 0 3 7 -2 1 0"),          # cap below n: the first two
        ("R 1 3  2 5 9  0 3 1  7 -2 8  1 0 1  3 0 0", "0 3 2 5 9 0 3 1 7 -2 8 1 0 1"),
        ("R 1 3  2 5 9  0 3 1  7 -2 8  1 0 1  5 0 0", "0 3 2 5 9 0 3 1 7 -2 8 1 0 1"),  # cap above n
        ("R 1 3  2 5 9  0 3 1  7 -2 8  1 0 1  2 1 0", f"{NULL} 57005"),                 # NULL columns with a cap
        ("R 1 3  2 5 9  0 3 1  7 -2 8  1 0 1  2 0 1", f"{NULL} 57005"),                 # NULL n_out
    ]
    # negative priorities travel as their unsigned form
    lines = [re.sub(r"-(\d+)", lambda m: str((1 << 32) - int(m.group(1))), c) for c, _ in cases]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert out[-1] == "ok"
    assert out[:-1] == [e for _, e in cases], [(c, o, e) for (c, e), o in zip(cases, out) if o != e]


# ---- where the new code sits -----------------------------------------------------------------------------------------------------------
def test_the_new_headers_are_listed_with_the_unit_that_includes_them():
    build = bsa.build
    csrc = os.path.join(ROOT, "batch-scheduler_amd", "csrc")
    assert [u for u in build.UNITS if "bs_preempt_clear.hpp" in build.UNITS[u]] == ["tu_preempt.hip"], "k_nc_resolve is emitted by one unit"
    assert '#include "bs_preempt_clear.hpp"' in open(os.path.join(csrc, "tu_preempt.hip")).read()
    assert "bs_preempt_clear_list.hpp" in build.UNITS["tu_preempt.hip"]
    assert "bs_nominated.hpp" not in build.UNITS["tu_preempt.hip"], "tu_preempt.hip reaches k_nc_list through bs_ctx.hpp's declaration only"
    for other in os.listdir(csrc):
        if other.endswith(".hip") and other != "tu_nominated.hip":
            assert '#include "bs_nominated.hpp"' not in open(os.path.join(csrc, other)).read(), f"{other} includes bs_nominated.hpp"
    lst = open(os.path.join(csrc, "bs_preempt_clear_list.hpp")).read()
    assert "hip" not in lst.split("#pragma once")[1].lower(), "the list header is plain C++"
    assert "nom_clear_list" in open(os.path.join(csrc, "bs_ctx.hpp")).read()
    assert "clear:" in open(os.path.join(csrc, "bs_preempt_clear.hpp")).read()


def test_new_kernels_use_no_scratch_and_keep_the_gang_resolves_waves():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from test_nominated_cpu import WAVES_BEFORE
    all_k = kernel_resources.resources()
    seen = {}
    for name, v in all_k.items():
        m = re.match(r"_ZN2bs\d+(k_\w+?)(?:ILi(\d+)E|E)", name)
        if not m:
            continue
        seen[m.group(1)] = seen.get(m.group(1), 0) + 1
        if not m.group(1).startswith("k_nc_"):
            continue
        assert v["scratch"] == 0, (name, v)
        if m.group(1) == "k_nc_resolve":
            S = int(m.group(2))
            waves = min(8, 512 // ((max(v["vgpr"], 1) + 7) // 8 * 8))
            assert waves >= WAVES_BEFORE["k_gang_resolve"][S], f"k_nc_resolve<{S}>: {v['vgpr']} VGPRs = {waves} waves, k_gang_resolve had {WAVES_BEFORE['k_gang_resolve'][S]}"
    assert {k: n for k, n in seen.items() if k.startswith("k_nc_")} == {"k_nc_resolve": 13, "k_nc_list": 1}, seen
    # the existing sets are what they were
    for k in ("k_pc_scan", "k_pc_resolve", "k_pc_nodes", "k_pc_boff", "k_pc_compact", "k_gang_resolve", "k_preempt_scan", "k_preempt_pick", "k_nm_move", "k_nm_gather"):
        assert seen.get(k) == 13, (k, seen.get(k))
    assert (seen.get("k_nm_mark"), seen.get("k_nm_chains")) == (1, 1)
    unit_of = lambda pat: {v["unit"] for k, v in all_k.items() if pat in k}
    assert unit_of("k_nc_list") == unit_of("k_nm_move") and unit_of("k_nc_resolve") == unit_of("k_gang_resolve")


def test_the_isa_summary_of_the_existing_kernels_is_committed():
    txt = open(os.path.join(ROOT, "profiles", "preempt_clear_isa_diff.txt")).read()
    assert "k_nc_resolve" in txt and "k_nc_list" in txt and re.search(r"differ \[\]", txt)
