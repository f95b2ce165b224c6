"""bs_bound_bind without a GPU: the array model (tests/bound_bind_ref.py) against a second statement — an object-by-object rebuild, a list
of pod objects per node re-sorted with Python's sorted on (-priority, start, id) — over seeded scenes that are not vacuous, the
hand-known answers of tests/golden/bound_bind_hand_kats.json, the model's refusals, the host-side argument checks alone under ASan +
UBSan, and the new unit's place in the build."""
import importlib
import json
import os
import subprocess
import types

import numpy as np
import pytest

import bound_apply_ref as bar
import bound_bind_ref as bbr
import wait_ref as wr

bsa = importlib.import_module("batch-scheduler_amd")
soa = bsa.soa
make_bound = bbr.make_bound
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENES = 200


def scene(seed):
    """a bound table, a wait table and a queue with the last pass's results; a call that binds rows of both kinds, at least two on one node,
    one of them tying a survivor on (priority, start)"""
    rng = np.random.default_rng(seed)
    S, n, g = int(seed % 3), int(rng.integers(2, 6)), int(rng.integers(1, 5))
    b = int(rng.integers(3, 14))
    bound = make_bound(rng.integers(0, n, b), rng.integers(0, 3, b), rng.integers(0, 3, b), S, rng, group=rng.integers(-2, g, b))
    btab = bar.Table(bound, S, n, bits=rng.integers(0, 2, b))
    w = int(rng.integers(2, 9))
    wtab = wr.load(n, g, S, rng.integers(0, n, w), rng.integers(0, g, w), rng.integers(-5, 1 << 40, (4 + S, w)), rng.integers(0, 1 << 4, w))
    dead = rng.permutation(w)[: int(rng.integers(0, w - 1))]
    wtab._keep(~np.isin(wtab.id, dead))
    P = int(rng.integers(3, 10))
    pods = types.SimpleNamespace(p=P, group=rng.integers(-2, g, P).astype(np.int32), req=rng.integers(-5, 1 << 40, (4 + S, P)).astype(np.int64),
                                 req_present=rng.integers(0, 1 << 4, P).astype(np.uint32))
    pod_node = rng.integers(-1, n, P).astype(np.int32)
    wait_node = np.where((pod_node >= 0) & (rng.random(P) < 0.3), pod_node, -1).astype(np.int32)
    # the call: some live wait rows, some placed pods that do not wait
    live = rng.permutation(wtab.id)
    nw = int(rng.integers(1, live.size + 1))
    wl = live[:nw]
    ok = np.nonzero((pod_node >= 0) & (wait_node < 0))[0]
    if ok.size == 0:
        pod_node[0], wait_node[0] = int(rng.integers(0, n)), -1
        ok = np.array([0])
    pl = rng.permutation(ok)[: int(rng.integers(1, ok.size + 1))]
    # two rows on one node: the first pod binds where the first wait row sits
    first_wait_node = int(wtab.node[np.nonzero(wtab.id == wl[0])[0][0]])
    pod_node[pl[0]] = first_wait_node
    cnt = nw + pl.size
    prio, start = rng.integers(0, 3, cnt).astype(np.int32), rng.integers(0, 3, cnt).astype(np.int64)
    on = np.nonzero(btab.node == first_wait_node)[0]
    if on.size == 0:                                          # a survivor to tie with
        btab.node[0] = first_wait_node
        on = np.array([0])
    prio[0], start[0] = btab.priority[on[0]], btab.start_ns[on[0]]
    pdb = rng.integers(0, 2, cnt) if seed % 4 else None
    return dict(S=S, n=n, g=g, btab=btab, wtab=wtab, pods=pods, pod_node=pod_node, wait_node=wait_node, wl=wl, pl=pl, prio=prio, start=start, pdb=pdb)


def rebuild(sc):
    """the second statement: pod objects per node, the new ones appended with fresh ids, every list re-sorted; the wait rows as objects"""
    bt, wt, S = sc["btab"], sc["wtab"], sc["S"]
    mask = (1 << S) - 1
    lists = [[] for _ in range(sc["n"])]
    for e in range(bt.count):
        lists[int(bt.node[e])].append(dict(id=int(bt.id[e]), prio=int(bt.priority[e]), start=int(bt.start_ns[e]), group=int(bt.group[e]),
                                           req=[int(x) for x in bt.req[:, e]], pres=int(bt.req_present[e]), pdb=int(bt.pdb[e])))
    wobj = [dict(id=int(wt.id[e]), node=int(wt.node[e]), group=int(wt.group[e]), req=[int(x) for x in wt.req[:, e]], pres=int(wt.req_present[e])) for e in range(wt.w)]
    new, i = [], 0
    for x in sc["wl"]:
        o = next(r for r in wobj if r["id"] == int(x))
        new.append((o["node"], dict(group=o["group"], req=list(o["req"]), pres=o["pres"])))
    for p in sc["pl"]:
        pres = int(sc["pods"].req_present[p]) & mask
        req = [int(sc["pods"].req[j, p]) for j in range(3)] + [1] + [int(sc["pods"].req[4 + s, p]) if (pres >> s) & 1 else 0 for s in range(S)]
        new.append((int(sc["pod_node"][p]), dict(group=int(sc["pods"].group[p]), req=req, pres=pres)))
    for i, (k, o) in enumerate(new):
        o.update(id=bt.ids + i, prio=int(sc["prio"][i]), start=int(sc["start"][i]), pdb=0 if sc["pdb"] is None else int(sc["pdb"][i] != 0))
        lists[k].append(o)
    lists = [sorted(lst, key=lambda o: (-o["prio"], o["start"], o["id"])) for lst in lists]
    gone = {int(x) for x in sc["wl"]}
    return lists, [r for r in wobj if r["id"] not in gone], [k for k, _ in new]


def test_the_model_against_the_object_rebuild_over_seeded_scenes():
    qualified = 0
    for seed in range(SCENES):
        sc = scene(seed)
        bt, wt = sc["btab"], sc["wtab"]
        # not vacuous: both kinds of row, a node with two or more inserts, an insert that ties a survivor
        node, _, _, _ = bbr.rows(wt, sc["wl"], sc["pods"], sc["pod_node"], sc["pl"], sc["S"])
        assert sc["wl"].size >= 1 and sc["pl"].size >= 1
        assert np.bincount(node, minlength=sc["n"]).max() >= 2
        tie = any(np.any((bt.node == node[i]) & (bt.priority == sc["prio"][i]) & (bt.start_ns == sc["start"][i])) for i in range(node.size))
        assert tie, seed
        qualified += 1
        want_lists, want_wait, want_nodes = rebuild(sc)
        ids0, w_ids0 = bt.ids, wt.ids
        out = bbr.bind(bt, wt, sc["n"], sc["g"], sc["wl"], sc["pl"], sc["prio"], sc["start"], sc["pdb"], sc["pods"], sc["pod_node"], sc["wait_node"])
        assert out["first_id"] == ids0 and out["node"].tolist() == want_nodes
        assert bt.ids == ids0 + node.size and wt.ids == w_ids0
        t = bt.table()
        flat = [(k, o) for k, lst in enumerate(want_lists) for o in lst]
        assert t["id"].tolist() == [o["id"] for _, o in flat] and t["node"].tolist() == [k for k, _ in flat]
        assert t["priority"].tolist() == [o["prio"] for _, o in flat] and t["start_ns"].tolist() == [o["start"] for _, o in flat]
        assert t["group"].tolist() == [o["group"] for _, o in flat] and t["pdb"].tolist() == [o["pdb"] for _, o in flat]
        assert t["req_present"].tolist() == [o["pres"] for _, o in flat] and t["req"].T.tolist() == [o["req"] for _, o in flat]
        assert wt.id.tolist() == [r["id"] for r in want_wait] and wt.node.tolist() == [r["node"] for r in want_wait]
        assert wt.group.tolist() == [r["group"] for r in want_wait] and wt.req.T.tolist() == [r["req"] for r in want_wait]
        assert wt.req_present.tolist() == [r["pres"] for r in want_wait]
    assert qualified == SCENES >= 200


def kat_state(s):
    n, g = s["n"], s["g"]
    bd = s["bound"]
    btab = bar.Table(make_bound(bd["node"], bd["priority"], bd["start_ns"], 0), 0, n)
    w = s["wait"]
    req = np.zeros((4, len(w["node"])), np.int64)
    req[0] = 100
    wtab = wr.load(n, g, 0, w["node"], w["group"], req, np.zeros(len(w["node"]), np.uint32))
    q = s["queue"]
    P = len(q["group"])
    preq = np.zeros((4, P), np.int64)
    preq[0] = 100
    pods = types.SimpleNamespace(p=P, group=np.array(q["group"], np.int32), req=preq, req_present=np.zeros(P, np.uint32))
    return btab, wtab, pods, np.array(q["pod_node"], np.int32), np.array(q["wait_node"], np.int32)


def hand_kats():
    with open(os.path.join(HERE, "golden", "bound_bind_hand_kats.json")) as f:
        return json.load(f)["scenes"]


@pytest.mark.parametrize("s", hand_kats(), ids=lambda s: s["name"][:40])
def test_hand_known_answers(s):
    btab, wtab, pods, pod_node, wait_node = kat_state(s)
    c, e = s["call"], s["expect"]
    before = (btab.table(), btab.ids, wtab.copy())
    if e["status"] != 0:
        with pytest.raises(bbr.BindError) as err:
            bbr.bind(btab, wtab, s["n"], s["g"], c["wait_ids"], c["pod_index"], c["priority"], c["start_ns"], c["pdb"], pods, pod_node, wait_node)
        assert err.value.status == e["status"]
        assert btab.ids == before[1] and btab.table()["id"].tolist() == before[0]["id"].tolist() and wtab.id.tolist() == before[2].id.tolist()
        return
    out = bbr.bind(btab, wtab, s["n"], s["g"], c["wait_ids"], c["pod_index"], c["priority"], c["start_ns"], c["pdb"], pods, pod_node, wait_node)
    t = btab.table()
    assert out["first_id"] == e["first_id"] and out["node"].tolist() == e["node_out"]
    assert t["id"].tolist() == e["id"] and t["node"].tolist() == e["node"] and t["group"].tolist() == e["group"] and t["pdb"].tolist() == e["pdb"]
    assert wtab.id.tolist() == e["wait_left"]
    assert bbr.max_group(-1, t["group"]) == e["max_group"]


def test_the_model_refuses_what_the_header_refuses_and_changes_nothing():
    sc = scene(7)
    bt, wt, n, g = sc["btab"], sc["wtab"], sc["n"], sc["g"]
    wl, pl = sc["wl"], sc["pl"]
    one = lambda k: (np.zeros(k, np.int32), np.zeros(k, np.int64))      # noqa: E731
    no_node = sc["pod_node"].copy()
    no_node[pl[0]] = -1
    waits = sc["wait_node"].copy()
    waits[pl[0]] = sc["pod_node"][pl[0]]
    dead = sorted(set(range(wt.ids)) - set(wt.id.tolist()))
    kw = dict(pods=sc["pods"], pod_node=sc["pod_node"], wait_node=sc["wait_node"])
    cases = [(bbr.STATE, lambda: bbr.bind(None, wt, n, g, wl[:1], [], *one(1), **kw)),
             (bbr.STATE, lambda: bbr.bind(bt, wt, n + 1, g, wl[:1], [], *one(1), **kw)),
             (bbr.STATE, lambda: bbr.bind(bt, None, n, g, wl[:1], [], *one(1), **kw)),
             (bbr.STATE, lambda: bbr.bind(bt, wt, n, g + 1, wl[:1], [], *one(1), **kw)),
             (bbr.STATE, lambda: bbr.bind(bt, wt, n, g, [], pl[:1], *one(1), window=False, **kw)),
             (bbr.STATE, lambda: bbr.bind(bt, wt, n, g, wl[:1], [], *one(1), single_rank=False, **kw)),
             (bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, wl[:1], [], None, None, **kw)),
             (bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, [wt.ids], [], *one(1), **kw)),
             (bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, [wl[0], wl[0]], [], *one(2), **kw)),
             (bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, [], [sc["pods"].p], *one(1), **kw)),
             (bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, [], [pl[0], pl[0]], *one(2), **kw)),
             (bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, [], pl[:1], *one(1), pods=sc["pods"], pod_node=no_node, wait_node=sc["wait_node"])),
             (bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, [], pl[:1], *one(1), pods=sc["pods"], pod_node=sc["pod_node"], wait_node=waits))]
    if dead:
        cases.append((bbr.INVALID, lambda: bbr.bind(bt, wt, n, g, dead[:1], [], *one(1), **kw)))
    before = (bt.table(), bt.ids, wt.copy())
    for want, fn in cases:
        with pytest.raises(bbr.BindError) as e:
            fn()
        assert e.value.status == want
        assert bt.ids == before[1] and bt.table()["id"].tolist() == before[0]["id"].tolist() and wt.id.tolist() == before[2].id.tolist()
    # the limits: the id space, and a node at BS_BOUND_MAX_PER_NODE (exactly the limit is fine)
    bt.ids = bbr.BOUND_MAX - 1
    with pytest.raises(bbr.BindError) as e:
        bbr.bind(bt, wt, n, g, wl[:1], pl[:1], *one(2), **kw)
    assert e.value.status == bbr.CAPACITY
    full = bar.Table(make_bound(np.zeros(2047, np.int64), np.zeros(2047), np.zeros(2047), 0), 0, 1)
    wt1 = wr.load(1, 1, 0, [0, 0], [0, 0])
    with pytest.raises(bbr.BindError) as e:
        bbr.bind(full, wt1, 1, 1, [0, 1], [], *one(2))
    assert e.value.status == bbr.CAPACITY and full.count == 2047 and wt1.w == 2
    assert bbr.bind(full, wt1, 1, 1, [1], [], *one(1))["first_id"] == 2047 and full.count == 2048 and wt1.id.tolist() == [0]
    assert bbr.bind(full, wt1, 1, 1, [], [], [], [])["first_id"] == 2048          # the empty call


# ---- the host-side argument checks, alone, under sanitizers ------------------------------------------------------------------------------
def test_argument_checks_under_sanitizers(tmp_path):
    """csrc/bs_bound_bind_check.hpp compiled alone with tests/native/bound_bind_check_main.cpp under ASan + UBSan, against the rules in Python"""
    exe = str(tmp_path / "bound_bind_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "bound_bind_check_main.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(41)
    lines, want = [], []
    for _ in range(200):
        nw, np_ = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        zw, zp, zpr, zst = (int(rng.random() < 0.2) for _ in range(4))
        lines.append(f"A {nw} {zw} {np_} {zp} {zpr} {zst}")
        want.append(1 if (nw and zw) or (np_ and zp) or ((nw or np_) and (zpr or zst)) else 0)
    for _ in range(400):
        ids, queue = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        rows = int(rng.integers(0, ids + 1))
        w = rng.integers(0, ids + 2, size=int(rng.integers(0, 6))).tolist() if rng.random() < 0.5 else rng.permutation(max(ids, 1))[: int(rng.integers(0, 6))].tolist()
        p = rng.integers(0, queue + 2, size=int(rng.integers(0, 6))).tolist() if rng.random() < 0.5 else rng.permutation(max(queue, 1))[: int(rng.integers(0, 6))].tolist()
        lines.append(" ".join(map(str, ["L", ids, rows, len(w), *w, queue, len(p), *p])))
        code = 0
        if any(x >= ids for x in w):
            code = 2
        elif len(w) > rows:
            code = 3
        elif any(x >= queue for x in p):
            code = 4
        elif len(p) > queue:
            code = 5
        want.append(code)
    for ids, nw, np_, limit, code in [(0, 0, 0, 1 << 24, 0), ((1 << 24) - 2, 1, 1, 1 << 24, 0), ((1 << 24) - 2, 2, 1, 1 << 24, 6), (5, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 24, 6),
                                      (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 6), (1 << 24, 0, 0, 1 << 24, 0), (1 << 24, 0, 1, 1 << 24, 6)]:
        lines.append(f"I {ids} {nw} {np_} {limit}")
        want.append(code)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == want
    assert all(want.count(c) >= 3 for c in (0, 1, 2, 3, 4, 6)), [want.count(c) for c in range(7)]


# ---- the new unit's place in the build ---------------------------------------------------------------------------------------------------
def test_the_bind_unit_is_built_linked_and_lists_every_header_it_reaches():
    build = importlib.import_module("batch-scheduler_amd.build")
    from test_build_units_cpu import closure
    assert "tu_bind.hip" in build.SOURCES
    reached = closure("tu_bind.hip")
    assert not reached - {os.path.normpath(h) for h in build.UNITS["tu_bind.hip"]}, sorted(reached)
    assert {"bs_bound_bind.hpp", "bs_bound_bind_check.hpp", "bs_bound_apply.hpp"} <= reached and "bs_wait.hpp" not in reached
    assert set(build.HEADERS) >= {"bs_bound_bind.hpp", "bs_bound_bind_check.hpp"}
    assert '#include "tu_bind.hip"' in open(os.path.join(build.CSRC, "bsched.hip")).read(), "the unity build includes the unit"


def test_the_bind_kernels_use_no_scratch_and_live_in_a_unit_of_their_own():
    """k_bb_rows / _scan1 / _scan2 / _scatter / _rank / _gather <S>, S = 0..12: no scratch, one unit, and that unit emits no k_wt_*, k_ba_* or
    k_seq_pass kernel"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources()
    res = {k: v for k, v in all_k.items() if "k_bb_" in k}
    assert len(res) == 6 * 13, sorted(res)
    for fam in ("k_bb_rows", "k_bb_scan1", "k_bb_scan2", "k_bb_scatter", "k_bb_rank", "k_bb_gather"):
        assert sum(fam in k for k in res) == 13, fam
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
    units = {v["unit"] for v in res.values()}
    assert len(units) == 1 and units.isdisjoint({v["unit"] for k, v in all_k.items() if "k_seq_pass" in k or "k_wt_" in k or "k_ba_" in k or "k_se_" in k})
