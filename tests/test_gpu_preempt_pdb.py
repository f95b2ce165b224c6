"""GPU tests of PDB-aware preemption (bs_bound_pdb_set / bs_preempt_pdb_read, steps 5 and 6 of bs_preempt_run, bs_preempt_commit's
library rule): everything bit-exact through the ABI against the numpy restatement of tests/preempt_pdb_ref.py (itself held against an
object-level restatement and hand known answers by tests/test_preempt_pdb_cpu.py).  Every random test asserts the conditions that keep
it from passing vacuously: the bits change the answer in at least a quarter of its scenes, and over its scene set the chosen node
differs, the victim order differs on an equal set, the chosen node has violations, top_priority is below the maximum victim priority
and earliest_start is not the first listed victim's, each at least once."""
import importlib

import numpy as np
import pytest

import preempt_commit_ref as pc
import preempt_pdb_ref as pp
import preempt_ref as pr
from preempt_scenes import groups_for

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth = bsa.soa, bsa.synth
OLD_FIELDS = ("node", "n_candidates", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start")


def _ctx(sc):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    return ctx


def _compare(got, exp, where, fields=pp.FIELDS):
    for f in fields:
        if not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(np.any((got[f] != exp[f]).reshape(len(got[f]), -1), axis=1))[0]
            i = int(bad[0])
            pytest.fail(f"{where}: {f} differs at preemptor {i} of {len(bad)} bad: got {got[f][i]} expected {exp[f][i]} "
                        f"(node {got['node'][i]} vs {exp['node'][i]})")


def _compare_state(ctx, exp, where):
    req, pres = ctx.read_node_requests()
    assert np.array_equal(pres, exp["pres"]), f"{where}: present bits"
    assert np.array_equal(req, exp["req"]), f"{where}: node requests"
    ids, nodes = ctx.read_bound()
    assert np.array_equal(ids, exp["bound_id"]) and np.array_equal(nodes, exp["bound_node"]), f"{where}: bound table"


def _run_np(sc, bits, cap):
    return pp.preempt_pdb_np(pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], bits), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], cap)


def _commit_np(sc, bits, cap, apply=False, assume=False):
    return pp.commit_pdb_np(pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], bits), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"],
                            sc["protected"], cap, apply, assume)


class _Seen:
    """the non-vacuity conditions over one test's scene set"""

    def __init__(self):
        self.seen, self.changed, self.total = set(), 0, 0

    def add(self, sc, res, plain, bits):
        e = pp.effects(sc, res, plain, bits)
        self.seen |= e
        self.changed += "changed" in e
        self.total += 1

    def check(self):
        assert 4 * self.changed >= self.total, f"the bits changed the answer in {self.changed} of {self.total} scenes"
        missing = [x for x in pp.EFFECTS if x not in self.seen]
        assert not missing, f"effects never seen over the scene set: {missing}"


# ---- the hand known answers
def test_hand_known_answers_on_device():
    for sc in pp.pdb_kats():
        s = pp.kat_pdb_scene(sc)
        with _ctx(s) as ctx:
            ctx.bound_pdb_set(s["violating"])
            got = ctx.preempt_commit(s["pod_index"], s["priority"], s["protected"], victim_cap=s["cap"])
            pp.check_pdb_kat(dict(res=got), sc, f"device commit {sc['name']}")
            if len(sc["expect"]) == 1:
                got = ctx.preempt(s["pod_index"], s["priority"], s["protected"], victim_cap=s["cap"])
                pp.check_pdb_kat(dict(res=got), sc, f"device run {sc['name']}")


# (S, nodes, bound pods per node, preemptors, groups, bit share)
CASES = [(0, 12, (5, 15), 30, 0, 0.6), (1, 40, (0, 12), 70, 6, 0.5), (4, 30, (2, 20), 24, 6, 0.5), (12, 25, (0, 10), 16, 0, 0.5),
         (0, 300, (0, 12), 130, 6, 0.5), (12, 200, (2, 20), 65, 6, 0.3)]


@pytest.mark.parametrize("S,n,per,q,groups,share", CASES)
def test_random_scenes_bit_exact_set_then_cleared(S, n, per, q, groups, share):
    seen = _Seen()
    for seed in range(6):
        sc, bits = pp.pdb_scene(9100 + 13 * seed + S + n, n, per, S, q, groups, share)
        where = f"S={S} n={n} q={q} groups={groups} seed={seed}"
        with _ctx(sc) as ctx:
            before = [ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap) for cap in (0, 3, 32)]
            ctx.bound_pdb_set(bits)
            for cap in (0, 3, 32):
                got = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap)
                _compare(got, _run_np(sc, bits, cap), f"{where} cap={cap}")
            seen.add(sc, got, before[2], bits)
            ctx.bound_pdb_set(None)                       # cleared: byte-identical to the answers before the bits were set
            for cap, b in zip((0, 3, 32), before):
                again = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap)
                for f in pp.FIELDS:
                    assert again[f].tobytes() == b[f].tobytes(), f"{where} cap={cap}: {f} after clearing the bits"
            assert not before[2]["n_pdb_violations"].any()
            _compare(before[2], pr.preempt_np(pr.Prep(sc["nodes"], sc["bound"], S), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"],
                                              sc["protected"], 32), f"{where} no bits", OLD_FIELDS)
    seen.check()


def _whole_node_preemptor(sc):
    """preemptor 0 at priority 5000 asks for all the cpu of node 0 that pods below 5000 hold, less 50 (below the smallest bound
    request): every potential victim has to go with or without bits, so the bits change nothing but the order of the list"""
    b, nd = sc["bound"], sc["nodes"]
    pot = (b.node == 0) & (b.priority < 5000)
    pi = int(sc["pod_index"][0])
    sc["pods"].req[:, pi] = 0
    sc["pods"].req[0, pi] = int(nd.allocatable[0, 0]) - (int(nd.requested[0, 0]) - int(b.req[0, pot].sum())) - 50
    sc["pods"].req_present[pi] = 0
    sc["priority"][0] = 5000
    return sc


@pytest.mark.parametrize("S", [1, 4])
def test_windowed_replay_more_than_64_potential_victims(S):
    """nodes with 100..300 bound pods: the victim list is replayed over several 64-entry windows, violating entries in every window"""
    seen = _Seen()
    for seed in range(6):
        n = (1, 2, 3)[seed % 3]
        sc, bits = pp.pdb_scene(400 + seed + S, n, (100, 300), S, 40, 0, 0.4, flagged=0.0, fit_density=1.0)
        if n == 1:
            sc = _whole_node_preemptor(sc)
        prep = pp.PdbPrep(sc["nodes"], sc["bound"], S, bits)
        assert prep.M > 64 and all(prep.viol[k, w:w + 64].any() for k in range(n) for w in range(0, int(prep.valid[k].sum()) - 63, 64))
        with _ctx(sc) as ctx:
            plain = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=300)
            ctx.bound_pdb_set(bits)
            got = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=300)
            _compare(got, _run_np(sc, bits, 300), f"windowed S={S} seed={seed}")
            assert got["n_victims"].max() > 64
            seen.add(sc, got, plain, bits)
            got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=300, apply=True)
            exp = _commit_np(sc, bits, 300, True, False)
            _compare(got, exp["res"], f"windowed commit S={S} seed={seed}")
            _compare_state(ctx, exp, f"windowed commit S={S} seed={seed}")
    seen.check()


def _reduced(sc, exp, bits):
    """the scene after APPLY: final node requests, the surviving entries (ascending caller id) and their bits"""
    nodes = soa.Nodes(sc["nodes"].allocatable, exp["req"], sc["nodes"].allocatable_present, exp["pres"], sc["nodes"].flags)
    keep = np.sort(exp["bound_id"]).astype(np.int64)
    b = sc["bound"]
    bound = soa.Bound(b.node[keep], b.priority[keep], b.start_ns[keep], b.group[keep], b.req[:, keep], b.req_present[keep])
    return dict(sc, nodes=nodes, bound=bound), keep, bits[keep]


def _map_ids(want, keep, cap):
    want["victims"] = np.where(np.arange(cap)[None] < np.minimum(want["n_victims"], cap)[:, None], keep[want["victims"]], 0).astype(np.uint32)
    return want


@pytest.mark.parametrize("S,n,per,q,groups,share", [(0, 12, (5, 15), 30, 0, 0.6), (1, 60, (0, 12), 70, 6, 0.5), (4, 30, (2, 20), 24, 6, 0.5),
                                                    (12, 120, (2, 14), 65, 6, 0.5)])
def test_commit_plan_apply_assume_and_the_state_after(S, n, per, q, groups, share):
    seen = _Seen()
    cap = 8
    for seed in range(4):
        sc, bits = pp.pdb_scene(5100 + 7 * seed + S + n, n, per, S, q, groups, share)
        sc2, _ = pp.pdb_scene(6100 + 7 * seed + S + n, n, per, S, q, groups, share)       # a second batch of preemptors (same queue size)
        for apply, assume in ((False, False), (True, False), (True, True)):
            where = f"S={S} n={n} q={q} seed={seed} apply={apply} assume={assume}"
            with _ctx(sc) as ctx:
                plain = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap)
                ctx.bound_pdb_set(bits)
                got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap, apply=apply, assume=assume)
                exp = _commit_np(sc, bits, cap, apply, assume)
                _compare(got, exp["res"], where)
                _compare_state(ctx, exp, where)
                if not apply:
                    seen.add(sc, got, plain, bits)
                    continue
                # the survivors kept their bits through the compaction: a second call on the applied state
                red, keep, kbits = _reduced(sc, exp, bits)
                red["pod_index"], red["priority"] = sc2["pod_index"], sc2["priority"]
                got2 = ctx.preempt(sc2["pod_index"], sc2["priority"], sc["protected"], victim_cap=cap)
                _compare(got2, _map_ids(_run_np(red, kbits, cap), keep, cap), f"{where}: bs_preempt_run on the applied state")
                # fresh bits in the OLD id space: evicted ids are skipped
                bits2 = pp.pdb_bits(seed + 77, sc["bound"], share)
                ctx.bound_pdb_set(bits2)
                ids, _ = ctx.read_bound()
                assert np.array_equal(np.sort(ids), keep)
                got3 = ctx.preempt_commit(sc2["pod_index"], sc2["priority"], sc["protected"], victim_cap=cap)
                want3 = _commit_np(red, bits2[keep], cap)["res"]
                _compare(got3, _map_ids(want3, keep, cap), f"{where}: bs_preempt_commit on the applied state, fresh bits")
    seen.check()


def test_full_size_cfg3_plan_by_relation():
    """one cfg3-sized plan: sampled slots equal bs_preempt_run on the state the earlier slots left, replayed on the host"""
    cfg = synth.CONFIGS["cfg3"]
    S = cfg["scalars"]
    sc, bits = pp.pdb_scene(20261016, cfg["nodes"], (20, 110), S, 1024, 200, 0.3, p=2000, classes=8, fit_density=0.95)
    cap = 64
    with _ctx(sc) as ctx:
        ctx.bound_pdb_set(bits)
        got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap)
    assert np.any(got["n_victims"] > 0) and np.any(got["n_pdb_violations"] > 0)
    vic = pc.victim_ids(got)
    assert len(vic) == len(set(vic)), "a bound pod is the victim of two slots"
    order = pc.slot_order(sc["priority"])
    req = sc["nodes"].requested.astype(np.int64).copy()
    pres = sc["nodes"].requested_present.copy()
    alive = np.ones(sc["bound"].b, bool)
    b = sc["bound"]
    sample = set(order[np.linspace(0, len(order) - 1, 6).astype(int)].tolist())
    for s, i in enumerate(order):
        if i in sample:
            nodes_s = soa.Nodes(sc["nodes"].allocatable, req.copy(), sc["nodes"].allocatable_present, pres.copy(), sc["nodes"].flags)
            keep = np.nonzero(alive)[0]
            bound_s = soa.Bound(b.node[keep], b.priority[keep], b.start_ns[keep], b.group[keep], b.req[:, keep], b.req_present[keep])
            with _ctx(dict(sc, nodes=nodes_s, bound=bound_s)) as c2:
                c2.bound_pdb_set(bits[keep])
                r = c2.preempt(sc["pod_index"][[i]], sc["priority"][[i]], sc["protected"], victim_cap=cap)
            r = _map_ids(r, keep, cap)
            for f in pp.FIELDS:
                assert np.array_equal(r[f][0], got[f][i]), f"slot {s} (preemptor {i}): {f} {r[f][0]} vs {got[f][i]}"
        k = int(got["node"][i])
        if k < 0:
            continue
        assert int(got["n_victims"][i]) <= cap
        v = pr.victims_of(got, i).astype(np.int64)
        assert int(bits[v].sum()) == int(got["n_pdb_violations"][i]) and np.all(alive[v]) and np.all(b.node[v] == k)
        nb = bits[v] != 0
        assert not np.any(nb[1:] & ~nb[:-1]), "violating victims are listed first"
        pi = int(sc["pod_index"][i])
        alive[v] = False
        for vv in v:
            req[:3, k] -= b.req[:3, vv]
            req[3, k] -= 1
            for t in range(S):
                if (int(b.req_present[vv]) >> t) & 1:
                    req[4 + t, k] = (req[4 + t, k] if (int(pres[k]) >> t) & 1 else 0) - b.req[4 + t, vv]
                    pres[k] |= np.uint32(1 << t)
        req[:3, k] += sc["pods"].req[:3, pi]
        req[3, k] += 1
        for t in range(S):
            if (int(sc["pods"].req_present[pi]) >> t) & 1:
                req[4 + t, k] = (req[4 + t, k] if (int(pres[k]) >> t) & 1 else 0) + sc["pods"].req[4 + t, pi]
                pres[k] |= np.uint32(1 << t)


def test_error_codes():
    sc, bits = pp.pdb_scene(4, 50, (0, 5), 1, 8, 4, 0.5, p=20)
    B = bsa.BsError
    with bsa.Context(scalar_lanes=1, device=0) as ctx:
        ctx.load_nodes(sc["nodes"], sc["fit"])
        ctx.load_groups(groups_for(sc))
        ctx.load_pods(sc["pods"])
        for call in (lambda: ctx.bound_pdb_set(bits), lambda: ctx.bound_pdb_set(None)):
            with pytest.raises(B) as e:
                call()                                                # before bs_bound_load
            assert e.value.status == -4
        npv = np.zeros(8, np.uint32)
        ptr = npv.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_uint32))
        assert ctx._lib.bs_preempt_pdb_read(ctx._h, 8, ptr) == -4   # no preemption call yet
        ctx.load_bound(sc["bound"])
        for wrong in (bits[:-1], np.concatenate([bits, [1]])):
            with pytest.raises(B) as e:
                ctx.bound_pdb_set(wrong)                              # b differs from the load's entry count
            assert e.value.status == -1
        ctx.bound_pdb_set(bits)
        got = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=4)
        _compare(got, _run_np(sc, bits, 4), "after the refused calls")
        assert ctx._lib.bs_preempt_pdb_read(ctx._h, 7, ptr) == -1    # count differs
        assert ctx._lib.bs_preempt_pdb_read(ctx._h, 8, None) == -1
        assert ctx._lib.bs_preempt_pdb_read(ctx._h, 8, ptr) == 0 and np.array_equal(npv, got["n_pdb_violations"])
        ctx.load_bound(sc["bound"])                                   # a load clears the bits
        got = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=4)
        _compare(got, _run_np(sc, None, 4), "bs_bound_load clears the bits")
        ctx.bound_pdb_set(bits)
        ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=4, apply=True)
        with pytest.raises(B) as e:
            ctx.bound_pdb_set(bits[: ctx.bound_count()] if ctx.bound_count() < bits.size else bits[:-1])   # the id space stays the load's
        assert e.value.status == -1
        ctx.bound_pdb_set(bits)
