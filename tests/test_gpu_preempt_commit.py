"""GPU tests of bs_preempt_commit / bs_bound_read (csrc/bs_preempt_commit.hpp): plans bit-exact against the numpy restatement of
tests/preempt_commit_ref.py (itself held against an object-level restatement and hand known answers by tests/test_preempt_commit_cpu.py),
the state BS_PREEMPT_APPLY / ASSUME leave (node requests, the bound table, and what later calls see), a full-size case checked by
relations, the flat form, error codes and the kernels' resources."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

import preempt_commit_ref as pc
import preempt_ref as pr
from preempt_scenes import groups_for, random_scene

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth = bsa.soa, bsa.synth
MAX_PER_NODE = 2048                                     # include/bsched.h BS_BOUND_MAX_PER_NODE
FIELDS = ("node", "n_candidates", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start")
HERE = os.path.dirname(os.path.abspath(__file__))


def commit_scene(seed, n, per_node, S, q, groups=9, p=None, **kw):
    """random_scene with q DISTINCT preemptors (a pod is nominated once)"""
    p = p or max(2 * q, 40)
    sc = random_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=groups, p=p, **kw)
    sc["pod_index"] = np.random.default_rng(seed).permutation(p)[:q].astype(np.uint32)
    return sc


def _ctx(sc):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    return ctx


def _expect(sc, cap, apply=False, assume=False):
    return pc.commit_np(pc.CommitPrep(sc["nodes"], sc["bound"], sc["S"]), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"],
                        sc["protected"], cap, apply, assume)


def _compare(got, exp, where):
    for f in FIELDS:
        if not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(np.any((got[f] != exp[f]).reshape(len(got[f]), -1), axis=1))[0]
            i = int(bad[0])
            pytest.fail(f"{where}: {f} differs at preemptor {i} of {len(bad)} bad: got {got[f][i]} expected {exp[f][i]} "
                        f"(node {got['node'][i]} vs {exp['node'][i]})")


def _compare_state(ctx, exp, where):
    req, pres = ctx.read_node_requests()
    assert np.array_equal(pres, exp["pres"]), f"{where}: present bits"
    bad = np.nonzero(np.any(req != exp["req"], axis=0))[0]
    assert bad.size == 0, f"{where}: node requests differ at nodes {bad[:8]}: {req[:, bad[0]]} vs {exp['req'][:, bad[0]]}"
    ids, nodes = ctx.read_bound()
    assert ctx.bound_count() == exp["bound_id"].size, f"{where}: bound count"
    assert np.array_equal(ids, exp["bound_id"]) and np.array_equal(nodes, exp["bound_node"]), f"{where}: bound table"


# ---- the hand known answers
def test_hand_known_answers_on_device():
    from preempt_commit_scenes import commit_kats, kat_commit_scene
    from test_preempt_commit_cpu import check_commit_kat
    for sc in commit_kats():
        s = kat_commit_scene(sc)
        with _ctx(s) as ctx:
            got = ctx.preempt_commit(s["pod_index"], s["priority"], s["protected"], victim_cap=s["cap"], apply=s["apply"], assume=s["assume"])
            req, pres = ctx.read_node_requests()
            ids, nodes = ctx.read_bound()
        check_commit_kat(dict(res=got, req=req, pres=pres, bound_id=ids, bound_node=nodes), sc, f"device {sc['name']}")


# (S, nodes, bound pods per node, preemptors)
CASES = [
    (0, 1, (0, 0), 1), (1, 1, (255, 257), 63), (4, 1, (1, 1), 64), (12, 3, (63, 65), 65),
    (0, 63, (63, 65), 64), (1, 64, (0, 1), 65), (4, 65, (30, 60), 300), (12, 64, (2, 9), 300),
    (0, 1000, (0, 3), 300), (1, 1000, (20, 40), 65), (4, 700, (5, 30), 63), (12, 500, (5, 12), 65),
    (1, 3, (MAX_PER_NODE, MAX_PER_NODE), 64), (0, 3000, (0, 2), 400),
]


@pytest.mark.parametrize("S,n,per,q", CASES)
def test_random_scenes_bit_exact_and_applied_state(S, n, per, q):
    sc = commit_scene(8100 + 17 * n + S + q, n=n, per_node=per, S=S, q=q, groups=9, fit_density=0.6)
    for apply, assume in ((False, False), (True, False), (True, True)):
        where = f"S={S} n={n} per={per} q={q} apply={apply} assume={assume}"
        with _ctx(sc) as ctx:
            got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=6, apply=apply, assume=assume)
            exp = _expect(sc, 6, apply, assume)
            _compare(got, exp["res"], where)
            _compare_state(ctx, exp, where)
    if n >= 64 and q >= 64:
        assert np.any(got["node"] >= 0)


@pytest.mark.parametrize("S", [0, 1, 4, 12])
def test_sparse_fit_flags_every_group_kind_and_extreme_priorities(S):
    lv = np.array([-(1 << 31), -(1 << 31) + 1, -5, 0, 7, (1 << 31) - 2, (1 << 31) - 1], np.int64)
    sc = commit_scene(41 + S, n=300, per_node=(0, 20), S=S, q=200, groups=5, fit_density=0.3, protected_share=0.5, flagged=0.2, levels=lv)
    with _ctx(sc) as ctx:
        got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=32, apply=True, assume=True)
        exp = _expect(sc, 32, True, True)
        _compare(got, exp["res"], f"sparse S={S}")
        _compare_state(ctx, exp, f"sparse S={S}")



# ---- the blob's two edges: no row for victims (victim_cap 0), and a context with no groups (the protected column clamped to one byte)
@pytest.mark.parametrize("cap,groups", [(0, 4), (0, 0), (6, 0)])
def test_no_room_for_victims_and_a_context_with_no_groups(cap, groups):
    from preempt_scenes import ungrouped_scene
    sc = commit_scene(8700, n=70, per_node=(2, 9), S=2, q=65, groups=4, p=70, fit_density=0.6)
    if not groups:
        sc = ungrouped_scene(sc)
    exp = _expect(sc, cap, True, True)
    assert np.any(exp["res"]["n_victims"] > 0), "the scene evicts nobody: APPLY has nothing to write"
    with _ctx(sc) as ctx:
        got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap, apply=True, assume=True)
        assert got["victims"].shape == (65, cap)
        _compare(got, exp["res"], f"cap {cap}, {groups} groups")
        _compare_state(ctx, exp, f"cap {cap}, {groups} groups")


def test_plan_only_changes_nothing_and_equals_apply_outputs():
    nodes, fit, groups, pods, _ = synth.make("tiny", "warm")
    bound, nodes = synth.make_bound(3, nodes.n, groups.g, (0, 20), 1)        # nearly full nodes: the plan evicts
    pidx = np.arange(0, pods.p, 3, dtype=np.uint32)
    prio = np.full(pidx.size, 1000, np.int32)
    prot = np.zeros(groups.g, np.uint8)
    outs, plans = [], []
    for flags in (None, 0, soa.PREEMPT_APPLY):
        with bsa.Context(scalar_lanes=1, device=0) as ctx:
            ctx.load_nodes(nodes, fit)
            ctx.load_groups(groups)
            ctx.load_pods(pods)
            ctx.load_bound(bound)
            req0, pres0 = ctx.read_node_requests()
            ids0, nd0 = ctx.read_bound()
            g0 = ctx.read_groups()
            if flags is not None:
                r = ctx.preempt_commit(pidx, prio, prot, victim_cap=8, apply=flags == soa.PREEMPT_APPLY)
                plans.append(r)
                assert np.any(r["node"] >= 0) and np.any(r["n_victims"] > 0)
                assert ctx.read_groups().state_equal(g0)
                assert ctx.read_pods().equal(pods)
            if flags == 0:
                req1, pres1 = ctx.read_node_requests()
                assert np.array_equal(req0, req1) and np.array_equal(pres0, pres1)
                ids1, nd1 = ctx.read_bound()
                assert np.array_equal(ids0, ids1) and np.array_equal(nd0, nd1) and ctx.bound_count() == bound.b
            if flags != soa.PREEMPT_APPLY:
                outs.append((ctx.batch(soa.STAGE_ALL), ctx.seq_run(soa.STAGE_PREFILTER)))
    for f in FIELDS:
        assert np.array_equal(plans[0][f], plans[1][f]), f
    for name in ("pf_code", "pf_first_k", "pf_leader", "fl_code", "fl_feasible", "fl_bitmap", "group_admit", "group_ready"):
        assert np.array_equal(getattr(outs[0][0], name), getattr(outs[1][0], name)), name
    for name in ("pf_code", "pod_node", "released_group", "released_pods"):
        assert np.array_equal(outs[0][1][name], outs[1][1][name]), name


def _reduced(sc, exp):
    """the scene after APPLY: final node requests, the surviving bound entries (ascending caller id: the same tie order)"""
    nodes = soa.Nodes(sc["nodes"].allocatable, exp["req"], sc["nodes"].allocatable_present, exp["pres"], sc["nodes"].flags)
    keep = np.sort(exp["bound_id"]).astype(np.int64)
    b = sc["bound"]
    bound = soa.Bound(b.node[keep], b.priority[keep], b.start_ns[keep], b.group[keep], b.req[:, keep], b.req_present[keep])
    return dict(sc, nodes=nodes, bound=bound), keep


def test_after_apply_preempt_run_sees_the_reduced_scene():
    sc = commit_scene(612, n=400, per_node=(3, 25), S=2, q=150, groups=6)
    with _ctx(sc) as ctx:
        ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=4, apply=True)
        exp = _expect(sc, 4, True, False)
        _compare_state(ctx, exp, "apply")
        sc2 = commit_scene(613, n=400, per_node=(3, 25), S=2, q=120, groups=6)
        got = ctx.preempt(sc2["pod_index"], sc2["priority"], sc["protected"], victim_cap=8)
    red, keep = _reduced(sc, exp)
    want = pr.preempt_np(pr.Prep(red["nodes"], red["bound"], 2), sc["fit"], sc["pods"], sc2["pod_index"], sc2["priority"], sc["protected"], 8)
    want["victims"] = np.where(np.arange(8)[None] < np.minimum(want["n_victims"], 8)[:, None], keep[want["victims"]], 0).astype(np.uint32)
    _compare(got, want, "bs_preempt_run after APPLY")
    assert np.any(got["n_victims"] > 0)


@pytest.mark.parametrize("assume", [False, True])
def test_after_apply_seq_run_equals_a_fresh_context(assume):
    nodes, fit, groups, pods, _ = synth.make("tiny", "warm")
    bound, nodes = synth.make_bound(5, nodes.n, groups.g, (2, 12), 1)
    pidx = np.arange(1, pods.p, 4, dtype=np.uint32)
    prio = (np.arange(pidx.size) % 3 * 1000 + 500).astype(np.int32)
    prot = np.zeros(groups.g, np.uint8)
    with bsa.Context(scalar_lanes=1, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        ctx.load_bound(bound)
        r = ctx.preempt_commit(pidx, prio, prot, victim_cap=4, apply=True, assume=assume)
        assert np.any(r["n_victims"] > 0)
        req, pres = ctx.read_node_requests()
        a = ctx.seq_run(soa.STAGE_PREFILTER)
        after_a = ctx.read_node_requests()
    fresh = soa.Nodes(nodes.allocatable, req, nodes.allocatable_present, pres, nodes.flags)
    with bsa.Context(scalar_lanes=1, device=0) as ctx:
        ctx.load_nodes(fresh, fit)
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        b = ctx.seq_run(soa.STAGE_PREFILTER)
        after_b = ctx.read_node_requests()
    for name in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(after_a[0], after_b[0]) and np.array_equal(after_a[1], after_b[1])


def test_full_size_cfg3_by_relation():
    cfg = synth.CONFIGS["cfg3"]
    S = cfg["scalars"]
    sc = commit_scene(20261016, n=cfg["nodes"], per_node=(20, 110), S=S, q=1024, groups=200, p=2000, classes=8, fit_density=0.95)
    cap = 64
    with _ctx(sc) as ctx:
        got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap)
    assert np.any(got["n_victims"] > 0) and np.any(got["node"] >= 0)
    vic = pc.victim_ids(got)
    assert len(vic) == len(set(vic)), "a bound pod is the victim of two slots"
    order = pc.slot_order(sc["priority"])
    prep = pr.Prep(sc["nodes"], sc["bound"], S)
    # replay slot by slot on the host: the working state (requests, surviving entries) and every nominee holds
    req = sc["nodes"].requested.astype(np.int64).copy()
    pres = sc["nodes"].requested_present.copy()
    alive = np.ones(sc["bound"].b, bool)
    b = sc["bound"]
    sample = set(order[np.linspace(0, len(order) - 1, 8).astype(int)].tolist())
    for s, i in enumerate(order):
        if i in sample:
            nodes_s = soa.Nodes(sc["nodes"].allocatable, req.copy(), sc["nodes"].allocatable_present, pres.copy(), sc["nodes"].flags)
            keep = np.nonzero(alive)[0]
            bound_s = soa.Bound(b.node[keep], b.priority[keep], b.start_ns[keep], b.group[keep], b.req[:, keep], b.req_present[keep])
            one = dict(sc, nodes=nodes_s, bound=bound_s)
            with _ctx(one) as c2:
                r = c2.preempt(sc["pod_index"][[i]], sc["priority"][[i]], sc["protected"], victim_cap=cap)
            r["victims"] = np.where(np.arange(cap)[None] < np.minimum(r["n_victims"], cap)[:, None], keep[r["victims"]], 0).astype(np.uint32)
            for f in FIELDS:
                assert np.array_equal(r[f][0], got[f][i]), f"slot {s} (preemptor {i}): {f} {r[f][0]} vs {got[f][i]}"
        k = int(got["node"][i])
        if k < 0:
            continue
        assert int(got["n_victims"][i]) <= cap
        pi = int(sc["pod_index"][i])
        for v in pr.victims_of(got, i):
            v = int(v)
            assert alive[v] and int(b.node[v]) == k
            alive[v] = False
            req[:3, k] -= b.req[:3, v]
            req[3, k] -= 1
            for t in range(S):
                if (int(b.req_present[v]) >> t) & 1:
                    req[4 + t, k] = (req[4 + t, k] if (int(pres[k]) >> t) & 1 else 0) - b.req[4 + t, v]
                    pres[k] |= np.uint32(1 << t)
        cur = req[:, k:k + 1].copy()
        for t in range(S):
            if not (int(pres[k]) >> t) & 1:
                cur[4 + t] = 0
        assert pr.holds_np(prep.alloc[:, k:k + 1], prep.apres[k:k + 1], cur, sc["pods"].req[:, pi].astype(np.int64),
                           int(sc["pods"].req_present[pi]), S)[0], f"slot {s}: the nominee does not hold on node {k}"
        req[:3, k] += sc["pods"].req[:3, pi]
        req[3, k] += 1
        for t in range(S):
            if (int(sc["pods"].req_present[pi]) >> t) & 1:
                req[4 + t, k] = (req[4 + t, k] if (int(pres[k]) >> t) & 1 else 0) + sc["pods"].req[4 + t, pi]
                pres[k] |= np.uint32(1 << t)


def test_flat_form_equals_struct_form():
    sc = commit_scene(12, n=100, per_node=(0, 15), S=1, q=65, groups=4)
    with _ctx(sc) as ctx:
        a = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=5)
        lib = ctx._lib
        u32, i32, i64 = (lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))), \
            (lambda x: x.ctypes.data_as(C.POINTER(C.c_int64)))
        q = len(sc["pod_index"])
        node, nc, nv = np.zeros(q, np.int32), np.zeros(q, np.uint32), np.zeros(q, np.uint32)
        vic, top, ssum, est = np.zeros((q, 5), np.uint32), np.zeros(q, np.int32), np.zeros(q, np.int64), np.zeros(q, np.int64)
        rc = lib.bs_preempt_commit_flat(ctx._h, soa.STAGE_PREFILTER, q, u32(sc["pod_index"]), i32(sc["priority"]),
                                        sc["protected"].ctypes.data_as(C.POINTER(C.c_uint8)), 0, 5, i32(node), u32(nc), u32(nv), u32(vic), i32(top),
                                        i64(ssum), i64(est))
        assert rc == 0
    b = dict(node=node, n_candidates=nc, n_victims=nv, victims=vic, top_priority=top, priority_sum=ssum, earliest_start=est)
    _compare(b, a, "flat form")


def test_error_codes_leave_the_state_alone():
    sc = commit_scene(4, n=50, per_node=(0, 5), S=1, q=8, groups=4, p=20)
    B = bsa.BsError
    with bsa.Context(scalar_lanes=1, device=0) as ctx:
        ctx.load_nodes(sc["nodes"], sc["fit"])
        ctx.load_groups(groups_for(sc))
        ctx.load_pods(sc["pods"])
        with pytest.raises(B) as e:
            ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"])   # no bound table
        assert e.value.status == -4
        with pytest.raises(B) as e:
            ctx.read_bound()
        assert e.value.status == -4
        ctx.load_bound(sc["bound"])
        req0, pres0 = ctx.read_node_requests()
        ids0, nd0 = ctx.read_bound()

        def unchanged():
            req, pres = ctx.read_node_requests()
            ids, nd = ctx.read_bound()
            assert np.array_equal(req, req0) and np.array_equal(pres, pres0) and np.array_equal(ids, ids0) and np.array_equal(nd, nd0)

        for args, kw, status in [
            (([3, 5, 3], [9, 8, 7]), dict(apply=True), -1),                                 # a pod index twice
            ((sc["pod_index"], sc["priority"]), dict(apply=False, assume=True), -1),      # ASSUME without APPLY
            (([25], [5]), dict(apply=True), -1),                                          # pod index >= p
            (([0], [5]), dict(apply=True, stages=soa.STAGE_FILTER), -1),
        ]:
            with pytest.raises(B) as e:
                ctx.preempt_commit(*args, sc["protected"], **kw)
            assert e.value.status == status, (args, kw)
            unchanged()
        q = len(sc["pod_index"])
        outs = [np.zeros(q, np.int32), np.zeros(q, np.uint32)]
        o = soa.PreemptOutStruct(outs[0].ctypes.data_as(C.POINTER(C.c_int32)), None, outs[1].ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, None)
        for flags in (4, 0x80000000, soa.PREEMPT_ASSUME):
            rc = ctx._lib.bs_preempt_commit(ctx._h, soa.STAGE_PREFILTER, q, sc["pod_index"].ctypes.data_as(C.POINTER(C.c_uint32)),
                                            sc["priority"].ctypes.data_as(C.POINTER(C.c_int32)), sc["protected"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                            flags, 0, C.byref(o))
            assert rc == -1, flags
            unchanged()
        ctx.set_shard(0, 2)
        with pytest.raises(B) as e:
            ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], apply=True)
        assert e.value.status == -4
        ctx.set_shard(0, 1)
        unchanged()
        nodes2 = soa.Nodes(sc["nodes"].allocatable[:, :40], sc["nodes"].requested[:, :40], sc["nodes"].allocatable_present[:40],
                           sc["nodes"].requested_present[:40], sc["nodes"].flags[:40])
        ctx.load_nodes(nodes2, soa.FitMasks.from_bool(sc["fit"].to_bool()[:, :40]))
        with pytest.raises(B) as e:
            ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], apply=True)   # the node list changed its count
        assert e.value.status == -4
        assert ctx.bound_count() == sc["bound"].b


def test_new_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import kernel_resources
    res = kernel_resources.resources()
    pcs = {k: v for k, v in res.items() if "k_pc_" in k}
    assert len(pcs) == 5 * 13, sorted(pcs)
    for k, v in pcs.items():
        assert v["scratch"] == 0, k
