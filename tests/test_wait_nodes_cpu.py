"""bs_wait_nodes_apply on the CPU: the model of tests/wait_nodes_ref.py (the header text taken literally) against its second statement (a
Python list of node identities under the deltas, one at a time) on seeded scenes, a numpy restatement of the device rule (the sorted
removed list, one binary search per row, the exclusive scan in blocks) against the model, the hand known answers of
tests/golden/wait_nodes_hand_kats.json, the refusals, and the new kernels' place in the build.  The host half of the call is
csrc/bs_bound_nodes_replay.hpp as it stands (tests/test_bound_nodes_cpu.py compiles it alone under the sanitizers); the call adds no host
header of its own.  No GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

import bound_nodes_ref as bn
import wait_nodes_ref as wn
import wait_ref as wr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U, A, R = wn.UPDATE, wn.APPEND, wn.REMOVE
SEEDS = range(400)
PROPS = ("removes_node_0", "removes_the_last_node", "adjacent_removes", "remove_then_append", "append_then_remove_cancels", "equal_count_with_a_remove",
         "updates_only", "down_to_zero_nodes", "empty_table", "down_to_an_empty_table", "two_groups_on_a_removed_node", "matched_wraps")


def scene(seed):
    """-> (table, matched, kind, index): a table on n nodes and a VALID delta list; seed % 8 steers the shape of the list"""
    rng = np.random.default_rng(seed)
    shape = seed % 8
    n = int(rng.integers(1, 9))
    g = int(rng.integers(1, 5))
    S = int(seed % 3)
    w = 0 if seed % 29 == 0 else int(rng.integers(1, 14))
    if seed % 31 == 1:                                      # every row on one node, which a list of this shape then removes
        node = np.zeros(w, np.int64)
    else:
        node = rng.integers(0, n, w)
    group = rng.integers(0, g, w)
    req = rng.integers(0, 1000, (4 + S, w))
    pres = rng.integers(0, 1 << S, w) if S else np.zeros(w, np.int64)
    tab = wr.load(n, g, S, node, group, req, pres)
    matched = rng.integers(0, 3, g).astype(np.uint32)
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
        put(R, rng.integers(0, n))
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
    if shape not in (5, 6, 7) and seed % 2:                 # a random tail
        for _ in range(int(rng.integers(0, 6))):
            k = int(rng.choice([U, A, R, R])) if cur else A
            put(k, rng.integers(0, cur) if k != A else 0)
    return tab, matched, kind, index


def properties(tab, matched, kind, index):
    new, n_new = wn.by_identity(tab.n, tab.node, kind, index)
    rem = wn.removed_sorted(tab.n, kind, index).tolist()
    gone = new < 0
    on = {}
    for k, x in zip(tab.node[gone].tolist(), tab.group[gone].tolist()):
        on.setdefault(k, set()).add(x)
    cancels, apps = False, 0
    cur = tab.n
    old_left = tab.n
    for k, i in zip(kind, index):
        if k == A:
            apps += 1
        elif k == R:
            if i >= old_left:
                cancels = True
                apps -= 1
            else:
                old_left -= 1
        cur += (k == A) - (k == R)
    first_r = kind.index(R) if R in kind else None
    return dict(
        removes_node_0=0 in rem, removes_the_last_node=tab.n - 1 in rem, adjacent_removes=any(b - a == 1 for a, b in zip(rem, rem[1:])),
        remove_then_append=first_r is not None and A in kind[first_r:], append_then_remove_cancels=cancels,
        equal_count_with_a_remove=n_new == tab.n and bool(rem), updates_only=bool(kind) and set(kind) == {U}, down_to_zero_nodes=n_new == 0,
        empty_table=tab.w == 0, down_to_an_empty_table=tab.w > 0 and bool(gone.all()), two_groups_on_a_removed_node=any(len(v) > 1 for v in on.values()),
        matched_wraps=any(int((tab.group[gone] == x).sum()) > int(matched[x]) for x in range(tab.g)))


def test_the_model_equals_the_identity_list_and_the_scenes_cover_the_cases():
    total = dict.fromkeys(PROPS, 0)
    for seed in SEEDS:
        tab, matched, kind, index = scene(seed)
        before, m0 = tab.copy(), matched.copy()
        for k, v in properties(tab, matched, kind, index).items():
            total[k] += int(bool(v))
        new, n_new = wn.by_identity(before.n, before.node, kind, index)
        out = wn.nodes_apply(tab, matched, kind, index)
        keep = new >= 0
        where = f"seed {seed}: {kind} {index}"
        assert tab.n == n_new and tab.ids == before.ids and tab.g == before.g, where
        assert np.array_equal(tab.id, before.id[keep]) and np.array_equal(tab.node, new[keep]) and np.array_equal(tab.group, before.group[keep]), where
        assert np.array_equal(tab.req, before.req[:, keep]) and np.array_equal(tab.req_present, before.req_present[keep]), where
        assert out["n"] == int((~keep).sum()) and np.array_equal(out["id"], before.id[~keep]) and np.array_equal(out["node"], before.node[~keep]), where
        assert np.array_equal(out["group"], before.group[~keep]) and np.array_equal(out["id"], np.sort(out["id"])), where
        want = (m0.astype(np.int64) - np.bincount(before.group[~keep], minlength=before.g)) & 0xFFFFFFFF
        assert np.array_equal(matched, want.astype(np.uint32)), where
        assert np.all(tab.node < max(n_new, 1)) and (tab.w == 0 or n_new > 0), where
    print(total)
    assert len(SEEDS) >= 300
    for k in PROPS:
        assert total[k] >= 8, (k, total)


def test_the_device_rule_equals_the_model():
    """the sorted removed list (two ways: from the identities, and csrc/bs_bound_nodes_replay.hpp restated), the search, the scan"""
    for seed in SEEDS:
        tab, matched, kind, index = scene(seed)
        rem = wn.removed_sorted(tab.n, kind, index)
        r2, app, n_new = bn.replay_sorted(tab.n, kind, index)
        assert rem.tolist() == r2, seed
        new, rows, left = wn.device_rule(tab, rem)
        out = wn.nodes_apply(tab, matched, kind, index)
        assert tab.n == n_new and left == out["n"], seed
        for f, v in tab.columns().items():
            assert np.array_equal(new[f], v), (seed, f)
        for f in ("id", "node", "group"):
            assert np.array_equal(rows[f], out[f]), (seed, f)


@pytest.mark.parametrize("rows", [1023, 1024, 1025, 2100])
def test_the_device_rule_across_scan_blocks(rows):
    rng = np.random.default_rng(rows)
    n, g = 40, 6
    tab = wr.load(n, g, 1, rng.integers(0, n, rows), rng.integers(0, g, rows), rng.integers(0, 99, (5, rows)), rng.integers(0, 2, rows))
    matched = rng.integers(0, 400, g).astype(np.uint32)
    kind, index = [R, R, A, R, R, U, R], [39, 0, 0, 17, 17, 3, 30]
    new, rows_out, left = wn.device_rule(tab, wn.removed_sorted(n, kind, index), cap=7)
    out = wn.nodes_apply(tab, matched, kind, index, n_expected=36)
    assert left == out["n"] > 100 and rows_out["id"].size == 7
    for f, v in tab.columns().items():
        assert np.array_equal(new[f], v), f
    for f in ("id", "node", "group"):
        assert np.array_equal(rows_out[f], out[f][:7]), f


@pytest.mark.parametrize("case", wn.hand_kats(), ids=lambda c: c["name"])
def test_hand_known_answers(case):
    assert case["pins"]
    t = case["table"]
    tab = wr.load(case["n"], case["g"], 0, t["node"], t["group"])
    matched = np.array(case["matched"], np.uint32)
    out = wn.nodes_apply(tab, matched, case["kind"], case["index"])
    e = case["expect"]
    assert tab.n == e["n_new"] and out["n"] == len(e["dropped"]["id"])
    for f in ("id", "node", "group"):
        assert out[f].tolist() == e["dropped"][f], f
    assert tab.id.tolist() == e["table_id"] and tab.node.tolist() == e["table_node"] and tab.group.tolist() == e["table_group"]
    assert matched.tolist() == e["matched"]


def test_the_hand_scenes_pin_what_the_issue_names():
    names = [c["name"] for c in wn.hand_kats()]
    for want in ("two_gangs_share_a_removed_node", "matched_zero_wraps", "cancelled_append", "equal_count"):
        assert want in names
    eq = next(c for c in wn.hand_kats() if c["name"] == "equal_count")
    assert eq["expect"]["n_new"] == eq["n"] and eq["expect"]["table_node"] != eq["table"]["node"][1:], "the answer differs from the unshifted table"
    wrap = next(c for c in wn.hand_kats() if c["name"] == "matched_zero_wraps")
    assert 0xFFFFFFFF in wrap["expect"]["matched"]


def test_model_errors_change_nothing():
    tab = wr.load(3, 2, 1, [0, 2, 1, 2], [0, 1, 0, 1], np.arange(20).reshape(5, 4), [1, 0, 1, 1])
    matched = np.array([2, 0], np.uint32)
    before = tab.copy()
    for kinds, idx, status, n_exp, g in (([3], [0], wr.INVALID, None, None), ([R], [3], wr.INVALID, None, None), ([U], [3], wr.INVALID, None, None),
                                         ([R, R, R, R], [0, 0, 0, 0], wr.INVALID, None, None), ([A, U], [0, 4], wr.INVALID, None, None),
                                         ([R, A, A, U], [2, 0, 0, 4], wr.INVALID, None, None), ([R], [0], wr.STATE, 3, None), ([], [], wr.STATE, 4, None),
                                         ([A, R], [0, 3], wr.STATE, 2, None), ([R], [0], wr.STATE, 2, 3)):
        with pytest.raises(wr.WaitError) as e:
            wn.nodes_apply(tab, matched, kinds, idx, n_expected=n_exp, g=g)
        assert e.value.status == status, (kinds, idx)
        assert (tab.n, tab.g, tab.ids) == (3, 2, 4) and matched.tolist() == [2, 0]
        assert all(np.array_equal(v, before.columns()[f]) for f, v in tab.columns().items())
    with pytest.raises(wr.WaitError) as e:
        wn.nodes_apply(None, matched, [], [])
    assert e.value.status == wr.STATE
    out = wn.nodes_apply(tab, matched, [], [], n_expected=3, g=2)
    assert out["n"] == 0 and all(np.array_equal(v, before.columns()[f]) for f, v in tab.columns().items())


def test_the_churn_cycle_scene_drops_rows_uses_appended_nodes_and_releases_a_gang(orc, soa):
    """the scene tests/test_gpu_wait_nodes.py replays on the device, on the model and the sequential oracle alone: it has what it is for"""
    import seq_expire_ref as ser
    nodes, fit, groups, pods1, pods2, steps = wn.churn_scene(soa)
    P = soa.STAGE_PREFILTER
    s1 = orc.seq_replay(nodes, fit, groups, pods1, P)
    st = ser.State.after_pass(nodes, fit, groups, pods1, s1)
    tab = wr.load(nodes.n, groups.g, nodes.lanes - 4)
    pk1 = wr.park(st, tab, pods1)
    assert pk1["n"] == 15 and sorted(set(tab.node.tolist())) == [0, 1, 2], "cycle 1: rows on nodes 0, 1, 2; nodes 3, 4, 5 hold none"
    nl = bn.NodeList(nodes, fit)
    nl.req, nl.rpres = st.requested.copy(), st.requested_present.copy()
    deltas = [nl.append(i) if k == A else nl.remove(i) for k, i in steps]
    m0 = st.matched.copy()
    out = wn.nodes_apply(tab, st.matched, [d.kind for d in deltas], [d.index for d in deltas], n_expected=nl.n)
    assert out["n"] == 6 and set(out["node"].tolist()) == {0} and len(set(out["group"].tolist())) == 2, "node 0's six rows, of two gangs"
    assert np.array_equal(st.matched, m0 - np.bincount(out["group"], minlength=3).astype(np.uint32)) and nl.n == 6 == tab.n
    queue2 = wr.second_queue(soa, pods1, pk1["pod"], pods2)
    mg = s1["groups"].copy()
    mg.matched[:] = st.matched
    s2 = orc.seq_replay(nl.nodes(), nl.fit(), mg, queue2, P, leader=s1["leader"])
    assert s2["n_released"] >= 1, "cycle 2 releases a gang whose rows the surgery renumbered"
    st2 = ser.State.after_pass(nl.nodes(), nl.fit(), mg, queue2, s2)
    assert np.any(st2.wait_node >= 2), "cycle 2 leaves pods waiting on the appended nodes"
    rel = wr.release(tab, s2["released_group"].tolist(), 6, 3)
    assert rel["n"] >= 1 and np.all(rel["node"] < 2), "the released rows name the old nodes' NEW indices"
    pk2 = wr.park(st2, tab, queue2)
    assert pk2["n"] >= 1 and np.any(tab.node >= 2), "rows on nodes beyond the old count"
    ex = wr.expire(st2, tab, sorted(set(tab.group.tolist())), deny=True)
    assert tab.w == 0 and ex["n"] >= 2


def test_the_by_node_kernels_use_no_scratch_and_live_in_the_wait_unit():
    """k_wn_map and k_wn_move<S>, S = 0..12: no scratch, in the unit of the k_wt_* kernels, which still emits neither k_seq_pass nor a k_se_* kernel"""
    build = importlib.import_module("batch-scheduler_amd.build")
    assert "bs_bound_nodes_replay.hpp" in build.UNITS["tu_wait.hip"], "the unit lists the replay header it reuses"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources()
    res = {k: v for k, v in all_k.items() if "k_wn_" in k}
    assert len(res) == 13 + 1, sorted(res)
    assert sum("k_wn_move" in k for k in res) == 13
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
    units = {v["unit"] for v in res.values()}
    assert units == {v["unit"] for k, v in all_k.items() if "k_wt_" in k}
    assert units.isdisjoint({v["unit"] for k, v in all_k.items() if "k_seq_pass" in k or "k_se_" in k})
