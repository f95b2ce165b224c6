"""bs_nominated_nodes_apply on the CPU: the model of tests/nominated_nodes_ref.py (the header text taken literally) against its second
statement (a Python list of node identities under the deltas, one at a time, rows as objects) on seeded scenes, a numpy restatement of the
device rule (the sorted removed list, one binary search per row, the window-wise stable compaction, a dropped row at e - survivors before
it) against the model, the hand known answers of tests/golden/nominated_nodes_hand_kats.json, the refusals, the host half of the call
(csrc/bs_nominated_nodes_check.hpp) compiled alone under the sanitizers, the new kernel's place in the build, and — on the model alone —
that the seeds tests/test_gpu_nominated_nodes.py replays on the device have what they are for.  No GPU."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bound_nodes_ref as bn
import nominated_nodes_ref as nn
import nominated_nodes_scenes as ns
import nominated_ref as nr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U, A, R = nn.UPDATE, nn.APPEND, nn.REMOVE
SEEDS = range(400)
PROPS = ("removes_node_0", "removes_the_last_node", "adjacent_removes", "remove_then_append", "append_then_remove_cancels", "equal_count_with_a_remove",
         "updates_only", "appends_only", "down_to_zero_nodes", "empty_table", "down_to_an_empty_table", "all_rows_on_the_removed_node")


def scene(seed):
    """-> (table, kind, index): a table of 0..13 rows on 1..8 nodes, S 0..2, and a VALID delta list; seed % 9 steers the shape of the list"""
    rng = np.random.default_rng(seed)
    shape = seed % 9
    n = int(rng.integers(1, 9))
    S = int(seed % 3)
    w = 0 if seed % 29 == 0 else int(rng.integers(1, 14))
    one = 0 if shape == 0 else n - 1 if shape == 1 else int(rng.integers(0, n))
    node = np.full(w, one, np.int64) if seed % 7 == 1 else rng.integers(0, n, w)        # (every row on one node, which shapes 0, 1, 3 remove)
    req = rng.integers(0, 1000, (4 + S, w))
    pres = rng.integers(0, 1 << S, w) if S else np.zeros(w, np.int64)
    tab = nr.NomTable(S)
    tab.load(n, node, rng.integers(-5, 50, w), req, pres)
    kind, index, cur = [], [], n

    def put(k, i=0):
        nonlocal cur
        kind.append(k)
        index.append(int(i))
        cur += (k == A) - (k == R)

    if shape == 0:
        put(R, 0)
    elif shape == 1:
        put(R, n - 1)
    elif shape == 2 and n >= 2:
        i = int(rng.integers(0, n - 1))
        put(R, i)
        put(R, i)                                           # old nodes i and i + 1
    elif shape == 3:
        put(R, one if seed % 7 == 1 else rng.integers(0, n))
        put(A)
    elif shape == 4:
        put(A)
        put(R, cur - 1)
    elif shape == 5:
        k = int(rng.integers(1, n + 1))
        for _ in range(k):
            put(R, rng.integers(0, cur)) if rng.random() < 0.5 and cur else put(A)
        while cur != n:
            put(R, rng.integers(0, cur)) if cur > n else put(A)
    elif shape == 6:
        for _ in range(int(rng.integers(0, 5))):
            put(U, rng.integers(0, n))
    elif shape == 7:
        while cur:
            put(R, rng.integers(0, cur))
    elif shape == 8:
        for _ in range(int(rng.integers(1, 5))):
            put(A)
    if shape not in (5, 6, 7, 8) and seed % 2:              # a random tail
        for _ in range(int(rng.integers(0, 6))):
            k = int(rng.choice([U, A, R, R])) if cur else A
            put(k, rng.integers(0, cur) if k != A else 0)
    return tab, kind, index


def properties(tab, kind, index):
    rem = nn.removed_sorted(tab.n, kind, index).tolist()
    gone = np.isin(tab.node, rem)
    _, _, n_new = nn.by_identity(tab.n, [], kind, index)
    cancels, old_left = False, tab.n
    for k, i in zip(kind, index):
        if k == R:
            if i >= old_left:
                cancels = True
            else:
                old_left -= 1
    first_r = kind.index(R) if R in kind else None
    return dict(
        removes_node_0=0 in rem, removes_the_last_node=tab.n - 1 in rem, adjacent_removes=any(b - a == 1 for a, b in zip(rem, rem[1:])),
        remove_then_append=first_r is not None and A in kind[first_r:], append_then_remove_cancels=cancels,
        equal_count_with_a_remove=n_new == tab.n and bool(rem), updates_only=bool(kind) and set(kind) == {U},
        appends_only=bool(kind) and set(kind) == {A}, down_to_zero_nodes=n_new == 0, empty_table=tab.id.size == 0,
        down_to_an_empty_table=tab.id.size > 0 and bool(gone.all()),
        all_rows_on_the_removed_node=tab.id.size > 1 and np.unique(tab.node).size == 1 and bool(gone.all()) and n_new > 0)


def _columns_equal(got: dict, exp: dict, where):
    for f in exp:
        assert np.array_equal(got[f], exp[f]), f"{where}: {f}: {np.asarray(got[f]).tolist()} vs {np.asarray(exp[f]).tolist()}"


# ---- the model against the second statement ----------------------------------------------------------------------------------------------
def test_the_model_equals_the_identity_list_and_the_scenes_cover_the_cases():
    total = dict.fromkeys(PROPS, 0)
    for seed in SEEDS:
        tab, kind, index = scene(seed)
        assert 1 <= tab.n <= 8 and tab.id.size <= 13 and tab.S <= 2
        before, ids0 = tab.read(), tab.ids
        for k, v in properties(tab, kind, index).items():
            total[k] += int(bool(v))
        kept, dropped, n_new = nn.by_identity(tab.n, nr.rows_as_objects(before, tab.S), kind, index)
        out = nn.nodes_apply(tab, kind, index)
        where = f"seed {seed}: {kind} {index}"
        assert tab.n == n_new and tab.ids == ids0, where
        _columns_equal(tab.read(), nr.objects_as_rows(kept, tab.S), where)
        assert out["n"] == len(dropped) and out["id"].tolist() == [r["id"] for r in dropped], where
        assert out["node"].tolist() == [r["node"] for r in dropped] and out["priority"].tolist() == [r["priority"] for r in dropped], where
        assert np.array_equal(out["id"], np.sort(out["id"])) and np.all(np.diff(tab.id.astype(np.int64)) > 0), where
        assert np.all(tab.node < max(n_new, 1)) and (tab.id.size == 0 or n_new > 0), where
    print(total)
    assert len(SEEDS) >= 400
    for k in PROPS:
        assert total[k] >= 8, (k, total)


# ---- the device rule against the model -------------------------------------------------------------------------------------------------------
def test_the_device_rule_equals_the_model():
    """the sorted removed list (two ways: from the identities, and csrc/bs_bound_nodes_replay.hpp restated), the search, the compaction"""
    for seed in SEEDS:
        tab, kind, index = scene(seed)
        rem = nn.removed_sorted(tab.n, kind, index)
        r2, app, n_new = bn.replay_sorted(tab.n, kind, index)
        assert rem.tolist() == r2, seed
        new, rows, left = nn.device_rule(tab.read(), rem)
        out = nn.nodes_apply(tab, kind, index)
        assert tab.n == n_new and left == out["n"], seed
        _columns_equal(new, tab.read(), f"seed {seed}")
        _columns_equal(rows, {f: out[f] for f in ("id", "node", "priority")}, f"seed {seed} dropped")


@pytest.mark.parametrize("rows", [1023, 1024, 1025, 2049])
def test_the_device_rule_across_windows(rows):
    rng = np.random.default_rng(rows)
    n = 40
    tab = nr.NomTable(1)
    tab.load(n, rng.integers(0, n, rows), rng.integers(0, 99, rows), rng.integers(0, 99, (5, rows)), rng.integers(0, 2, rows))
    kind, index = [R, R, A, R, R, U, R], [39, 0, 0, 17, 17, 3, 30]
    new, rows_out, left = nn.device_rule(tab.read(), nn.removed_sorted(n, kind, index), cap=7)
    out = nn.nodes_apply(tab, kind, index, n_expected=36)
    assert left == out["n"] > 100 and rows_out["id"].size == 7
    _columns_equal(new, tab.read(), f"{rows} rows")
    _columns_equal(rows_out, {f: out[f][:7] for f in ("id", "node", "priority")}, f"{rows} rows dropped")


# ---- the hand known answers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", nn.hand_kats(), ids=lambda c: c["name"])
def test_hand_known_answers(case):
    assert case["pins"]
    tab = nn.kat_table(case)
    lanes = tab.read()
    out = nn.nodes_apply(tab, case["kind"], case["index"])
    e = case["expect"]
    assert tab.n == e["n_new"] and out["n"] == len(e["dropped"]["id"])
    for f in ("id", "node", "priority"):
        assert out[f].tolist() == e["dropped"][f], f
    assert tab.id.tolist() == e["table_id"] and tab.node.tolist() == e["table_node"] and tab.prio.tolist() == e["table_priority"]
    assert tab.ids == len(case["table"]["node"]), "bs_nominated_ids is unchanged"
    assert np.array_equal(tab.req, lanes["req"][:, e["table_id"]]), "a survivor keeps its request lanes"


def test_the_hand_scenes_pin_what_the_issue_names():
    kats = {c["name"]: c for c in nn.hand_kats()}
    assert len(kats) >= 8
    for want in ("remove_node_0", "remove_the_last_node", "adjacent_removes", "equal_count", "cancelled_append", "appends_only", "updates_only",
                 "down_to_zero_nodes", "empty_table", "down_to_an_empty_table"):
        assert want in kats
    eq = kats["equal_count"]
    assert eq["expect"]["n_new"] == eq["n"] and eq["expect"]["table_node"] != eq["table"]["node"][1:], "the answer differs from the unshifted table"
    assert kats["appends_only"]["expect"]["n_new"] > kats["appends_only"]["n"] and not kats["appends_only"]["expect"]["dropped"]["id"]


# ---- the refusals of the model ---------------------------------------------------------------------------------------------------------------
def test_model_errors_change_nothing():
    tab = nr.NomTable(1)
    tab.load(3, [0, 2, 1, 2], [5, 6, 7, 8], np.arange(20).reshape(5, 4), [1, 0, 1, 1])
    before = tab.read()
    for kinds, idx, code, n_exp in (([3], [0], "BS_ERR_INVALID", None), ([R], [3], "BS_ERR_INVALID", None), ([U], [3], "BS_ERR_INVALID", None),
                                    ([R, R, R, R], [0, 0, 0, 0], "BS_ERR_INVALID", None), ([A, U], [0, 4], "BS_ERR_INVALID", None),
                                    ([R, A, A, U], [2, 0, 0, 4], "BS_ERR_INVALID", None), ([R], [0], "BS_ERR_STATE", 3), ([], [], "BS_ERR_STATE", 4),
                                    ([A, R], [0, 3], "BS_ERR_STATE", 2)):
        with pytest.raises(nr.NomRefused) as e:
            nn.nodes_apply(tab, kinds, idx, n_expected=n_exp)
        assert e.value.code == code, (kinds, idx)
        assert (tab.n, tab.ids) == (3, 4)
        _columns_equal(tab.read(), before, f"{kinds} {idx}")
    for no_table in (None, nr.NomTable(0)):
        with pytest.raises(nr.NomRefused, match="BS_ERR_STATE"):
            nn.nodes_apply(no_table, [], [])
    with pytest.raises(nr.NomRefused, match="BS_ERR_STATE"):
        nn.nodes_apply(tab, [], [], n_expected=3, single_rank=False)
    out = nn.nodes_apply(tab, [], [], n_expected=3)
    assert out["n"] == 0
    _columns_equal(tab.read(), before, "count == 0")
    # a dropped id is dead exactly as one removed by bs_nominated_apply
    nn.nodes_apply(tab, [R], [2])
    with pytest.raises(nr.NomRefused, match="BS_ERR_INVALID"):
        tab.apply([1], [], [], [], None)
    assert tab.id.tolist() == [0, 2] and tab.ids == 4


# ---- the host half, alone, under sanitizers ----------------------------------------------------------------------------------------------------
OK, NULL, DELTA, COUNT = range(4)


def test_host_half_under_sanitizers(tmp_path):
    """csrc/bs_nominated_nodes_check.hpp (over bs_bound_nodes_replay.hpp) compiled alone with tests/native/nominated_nodes_check_main.cpp
    under ASan + UBSan: every refusal, NULL with count 0 and cap 0, the replay of the 400 seeded lists against the Python restatement, when
    the device has to run, and the live ids after a drop"""
    exe = str(tmp_path / "nominated_nodes_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "nominated_nodes_check_main.cpp"), "-o", exe], check=True)
    lst = lambda v: " ".join(str(int(x)) for x in v)
    cases = [
        ("C 3 3 5 0 1   0 1 0", [OK, 3, 0, 0, 0]),                       # count == 0, NULL lists, cap == 0 with NULL arrays
        ("C 3 3 5 0 0   4 0 0", [OK, 3, 0, 0, 0]),
        ("C 3 3 5 0 0   4 1 0", [NULL]),                                 # a NULL result array with cap > 0
        ("C 3 3 5 0 0   0 1 1", [NULL]),                                 # NULL n_out
        ("C 3 2 5 1 1   0 1 0", [NULL]),                                 # NULL kind / index with count > 0
        ("C 3 2 5 1 0 3 0   0 1 0", [DELTA]),                            # a kind outside the three
        ("C 3 2 5 1 0 2 3   0 1 0", [DELTA]),                            # REMOVE at the count
        ("C 3 3 5 1 0 0 3   0 1 0", [DELTA]),                            # UPDATE at the count
        ("C 3 4 5 2 0 1 0 0 4   0 1 0", [DELTA]),                        # ... one beyond the appended node
        ("C 3 4 5 2 0 1 0 0 3   0 1 0", [OK, 4, 1, 1, 0]),               # ... the appended node itself; appends only: the device runs
        ("C 3 4 0 2 0 1 0 0 3   0 1 0", [OK, 4, 1, 0, 0]),               # ... but not for an empty table
        ("C 3 3 5 1 0 2 0   0 1 0", [COUNT]),                            # the replay ends at 2, the list holds 3
        ("C 3 4 5 0 1   0 1 0", [COUNT]),                                # count == 0 with counts that differ
        ("C 3 3 5 2 0 2 1 0 0   0 1 0", [OK, 3, 1, 1, 1, 0]),            # equal count with a remove: the device runs
        ("C 3 3 5 2 0 1 2 0 3   0 1 0", [OK, 3, 0, 0, 0]),               # a cancelled append: nothing to do
        ("C 3 3 5 2 0 0 0 2 0   0 1 0", [OK, 3, 0, 0, 0]),               # UPDATEs only
        ("C 2 0 3 2 0 2 2 0 0   3 0 0", [OK, 0, 0, 1, 2, 0, 1]),         # down to zero nodes
        ("L 5 0 2 4 6 9   0", [5, 0, 2, 4, 6, 9]),
        ("L 5 0 2 4 6 9   2 0 9", [3, 2, 4, 6]),
        ("L 5 0 2 4 6 9   5 0 2 4 6 9", [0]),
        ("L 0   0", [0]),
    ]
    for seed in SEEDS:
        tab, kind, index = scene(seed)
        r, app, n_new = bn.replay_sorted(tab.n, kind, index)
        moves = int(tab.id.size > 0 and (bool(r) or n_new != tab.n))
        null = 0 if kind else 1
        cases.append((f"C {tab.n} {n_new} {tab.id.size} {len(kind)} {null} {lst(kind)} {lst(index)} 0 1 0", [OK, n_new, app, moves, len(r)] + r))
    out = subprocess.run([exe], input="\n".join(c for c, _ in cases) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert out[-1] == "ok" and len(out) == len(cases) + 1
    for (c, e), line in zip(cases, out):
        assert [int(x) for x in line.split()] == e, (c, line)


# ---- where the new code sits -----------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_lives_in_the_nominated_unit():
    """k_nn_move<S>, S = 0..12: no scratch, emitted by the unit of the k_nm_* kernels alone; the unit lists the headers it reuses"""
    build = importlib.import_module("batch-scheduler_amd.build")
    assert {"bs_bound_nodes_replay.hpp", "bs_nominated_nodes_check.hpp"} <= set(build.UNITS["tu_nominated.hip"])
    assert [u for u in build.SOURCES if "bs_nominated_nodes_check.hpp" in build.UNITS[u]] == ["tu_nominated.hip"]
    check = open(os.path.join(ROOT, "batch-scheduler_amd", "csrc", "bs_nominated_nodes_check.hpp")).read()
    assert "hip" not in check.split("#pragma once")[1].lower(), "the check header is plain C++"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources()
    res = {k: v for k, v in all_k.items() if re.search(r"\d+k_nn_", k)}
    assert len(res) == 13 and sum(bool(re.search(r"\d+k_nn_moveILi\d+E", k)) for k in res) == 13, sorted(res)
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
    assert {v["unit"] for v in res.values()} == {v["unit"] for k, v in all_k.items() if re.search(r"\d+k_nm_", k)}
    assert sum(bool(re.search(r"\d+k_nm_moveILi\d+E", k)) for k in all_k) == 13, "k_nm_move got no new template parameter"


# ---- the seeds of the GPU tests, verified on the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", sorted(ns.TWIN_SEEDS))
def test_the_twin_scenes_drop_rows_move_survivors_and_their_rows_change_every_answer(S):
    w, steps = ns.twin_scene(S)
    before = w.rows()
    _, kinds, idx = w.cut(steps)
    out = w.follow(kinds, idx)
    after = w.rows()
    assert out["n"] >= 1, "no row is dropped"
    assert np.any(after["node"] != before["node"][np.isin(before["id"], after["id"])]), "no survivor changes its node index"
    assert after["id"].size >= 1 and w.nl.n == w.tab.n
    for mode in ns.MODES:
        assert nr.changed(w.expect_raw(mode)["res"], w.expect_raw(mode, rows=None)["res"]), f"S={S} {mode}: the surviving rows change no answer"


def test_the_equal_count_scene_puts_rows_on_the_wrong_nodes_without_the_call():
    """a REMOVE and an APPEND in one batch keep the count; without the call the rows would sit on the wrong nodes and change the answers"""
    w, _ = ns.twin_scene(2)
    before = w.rows()
    holders = np.unique(before["node"])
    _, kinds, idx = w.cut([(R, int(holders[0])), (A, 3)])
    assert w.nl.n == 48, "the count is kept"
    stale = {f: v.copy() for f, v in before.items()}
    out = w.follow(kinds, idx)
    after = w.rows()
    assert out["n"] >= 1 and w.tab.n == 48
    assert not np.array_equal(after["node"], stale["node"][np.isin(stale["id"], after["id"])]), "the rows do not move"
    assert any(nr.changed(w.expect_raw(m)["res"], w.expect_raw(m, rows=stale)["res"]) for m in ns.MODES), "the stale rows give the same answers"


def test_the_fuzz_seeds_drop_rows_and_take_every_step_kind():
    drops, kinds = 0, dict.fromkeys(ns.FUZZ_KINDS, 0)
    assert len(ns.FUZZ_SEEDS) == 20
    for seed in ns.FUZZ_SEEDS:
        steps = 0
        for item in ns.fuzz_run(seed):
            if item[0] == "start":
                continue
            steps += 1
            kinds[item[0]] += 1
            if item[0] == "surgery":
                drops += item[4]["n"]
        assert steps == 12
    assert drops >= 20 and all(kinds.values()), (drops, kinds)


def test_the_appends_only_scene_puts_decisive_rows_beyond_the_old_count():
    w, steps, rows_for = ns.appends_scene()
    _, kinds, idx = w.cut(steps)
    assert set(kinds) == {A} and w.follow(kinds, idx)["n"] == 0 and w.nl.n == 700
    args = rows_for(w)
    assert min(args[2]) >= 24 and max(args[2]) == 699, "every new row sits on an appended node"
    before = {m: w.expect_raw(m)["res"] for m in ns.MODES}
    w.tab.apply(*args, w.sc["pods"])
    for m in ns.MODES:
        assert nr.changed(w.expect_raw(m)["res"], before[m]), f"{m}: the rows on the appended nodes change no answer"
