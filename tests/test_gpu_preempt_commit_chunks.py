"""GPU tests of k_pc_resolve (csrc/bs_preempt_commit.hpp) where node chunks hold several nodes: the record's fallback entries 1..3, the
rescan of a chunk whose recorded nodes are all dirty, several rescans in one slot, the rescan list's spill, the n_candidates correction,
and the same under PDB bits (the widened key, k_pc_scan's early exit on four victim-free nodes).  With one node a chunk — the shipped
geometry (csrc/bs_preempt_geom.hpp) of almost every scene of tests/test_gpu_preempt_commit.py and tests/test_gpu_preempt_pdb.py — none of
that does any work.

Everything is compared bit-exact with the numpy restatements (tests/preempt_commit_ref.py, tests/preempt_pdb_ref.py).  Every test FIRST
asserts, on the oracle-side classifier's counts (tests/preempt_commit_paths.py: the reference plan and the geometry, never device
output), that its scene makes the resolve take the paths the test is about; it prints those counts and its wall times (pytest -s).
Chunks of several nodes come either from the shipped geometry at a large queue, or from the test hook BS_TEST_PC_CHUNK_NODES (read at
context creation), which changes the chunk split and nothing else.

A mismatch is located with paths.classify(sc, exp["res"], chunk_nodes, detail=True)["slots"][slot]: the chunks that slot takes from a
later entry, rescans, or answers from the dirty list alone.

Two scratch mutations of k_pc_resolve, each run once when this file was written: (i) stage A looks at entry 0 of a record only — 16 of
these 17 tests fail (all but bs_preempt_run's), tests/test_gpu_preempt_commit.py notices in two S = 0 cases; (ii) the rescan of a chunk
without a clean entry is skipped — 13 fail (the large-queue cases with 4, 32 and 0 rescans pass: no rescanned chunk held a slot's best
node), tests/test_gpu_preempt_commit.py passes whole."""
import importlib
import time

import numpy as np
import pytest

import preempt_commit_paths as paths
import preempt_commit_ref as pc
import preempt_pdb_ref as pp
import preempt_ref as pr
from preempt_scenes import groups_for, random_scene

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa = bsa.soa
HOOK = "BS_TEST_PC_CHUNK_NODES"
FIELDS = ("node", "n_candidates", "n_victims", "victims", "top_priority", "priority_sum", "earliest_start")


def pc_threads(S: int) -> int:
    """pc_threads<S>() of csrc/bs_preempt_commit.hpp: k_pc_resolve's workgroup = the entries of its rescan list"""
    return 256 if S >= 12 else 512


def commit_scene(seed, n, per_node, S, q, groups=9, p=None, **kw):
    """random_scene with q DISTINCT preemptors (tests/test_gpu_preempt_commit.py's)"""
    p = p or max(2 * q, 40)
    sc = random_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=groups, p=p, **kw)
    sc["pod_index"] = np.random.default_rng(seed).permutation(p)[:q].astype(np.uint32)
    return sc


def _ctx(sc, bits=None):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    if bits is not None:
        ctx.bound_pdb_set(bits)
    return ctx


def _expect(sc, cap, apply=False, assume=False, bits=None):
    if bits is None:
        return pc.commit_np(pc.CommitPrep(sc["nodes"], sc["bound"], sc["S"]), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"],
                            sc["protected"], cap, apply, assume)
    return pp.commit_pdb_np(pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], bits), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"],
                            sc["protected"], cap, apply, assume)


def _compare(got, exp, where, fields=FIELDS):
    for f in fields:
        if not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(np.any((got[f] != exp[f]).reshape(len(got[f]), -1), axis=1))[0]
            i = int(bad[0])
            pytest.fail(f"{where}: {f} differs at preemptor {i} of {len(bad)} bad: got {got[f][i]} expected {exp[f][i]} "
                        f"(node {got['node'][i]} vs {exp['node'][i]})")


def _state(ctx):
    req, pres = ctx.read_node_requests()
    ids, nodes = ctx.read_bound()
    return req, pres, ids, nodes


def _compare_state(ctx, exp, where):
    req, pres, ids, nodes = _state(ctx)
    assert np.array_equal(pres, exp["pres"]), f"{where}: present bits"
    bad = np.nonzero(np.any(req != exp["req"], axis=0))[0]
    assert bad.size == 0, f"{where}: node requests differ at nodes {bad[:8]}: {req[:, bad[0]]} vs {exp['req'][:, bad[0]]}"
    assert ctx.bound_count() == exp["bound_id"].size, f"{where}: bound count"
    assert np.array_equal(ids, exp["bound_id"]) and np.array_equal(nodes, exp["bound_node"]), f"{where}: bound table"


def _commit(ctx, sc, cap, apply=False, assume=False):
    t0 = time.perf_counter()
    got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=cap, apply=apply, assume=assume)
    return got, time.perf_counter() - t0


# ---- a. the shipped geometry at a large queue: (S, nodes, bound pods per node, preemptors, fit density, chunk_nodes as shipped)
LARGE_Q = [(4, 400, (1, 6), 4096, 0.6, 7), (12, 320, (0, 3), 4096, 0.6, 5), (1, 257, (2, 5), 8192, 0.9, 9), (4, 20000, (1, 3), 256, 0.6, 20),
           (1, 640, (0, 4), 2048, 0.6, 5)]


@pytest.mark.parametrize("S,n,per,q,fit,cn", LARGE_Q)
def test_shipped_geometry_large_queue_fallback_entries_and_rescans(S, n, per, q, fit, cn, monkeypatch):
    """classifier counts when written ((later entry, rescans, most in one slot), by case): (1552, 224, 4), (305, 4, 1), (2031, 11180, 19),
    (1165, 32, 3), (3353, 0, 0); n_candidates corrected in 3688 / 2579 / 7598 / 225 / 1916 slots"""
    monkeypatch.delenv(HOOK, raising=False)
    sc = commit_scene(8100 + 17 * n + S + q, n=n, per_node=per, S=S, q=q, groups=9, fit_density=fit)
    t0 = time.perf_counter()
    assert paths.geometry(n, count=q)[2] == cn
    exp = _expect(sc, 6, True, True)
    cl = paths.classify(sc, exp["res"], cn)
    t_ref = time.perf_counter() - t0
    print(f"\nS={S} n={n} q={q}: {paths.summary(cl)}")
    assert cl["later"] > 0 and cl["ncand_corrected"] > 0 and cl["chosen_dirty"] > 0
    if n != 640:
        assert cl["rescans"] > 0
    if S == 4:
        assert cl["rescans_max"] >= 2
    if n == 257:
        assert cl["rescans_max"] >= 10
    where = f"S={S} n={n} per={per} q={q}"
    with _ctx(sc) as ctx:
        before = _state(ctx)
        got, t_plan = _commit(ctx, sc, 6)
        _compare(got, exp["res"], where + " plan")
        assert all(np.array_equal(a, b) for a, b in zip(before, _state(ctx))), where + ": a plan changes nothing"
        got, t_apply = _commit(ctx, sc, 6, True, True)
        _compare(got, exp["res"], where + " apply+assume")
        _compare_state(ctx, exp, where + " apply+assume")
    print(f"oracle + classifier {t_ref:.2f} s; device calls: plan {t_plan * 1e3:.1f} ms, apply+assume {t_apply * 1e3:.1f} ms")
    if S == 12:
        exp = _expect(sc, 6, True, False)
        with _ctx(sc) as ctx:
            got, _ = _commit(ctx, sc, 6, True, False)
            _compare(got, exp["res"], where + " apply")
            _compare_state(ctx, exp, where + " apply")


# ---- b. the answer does not depend on the chunk split
GEOM_SEEDS = {0: 700, 1: 714, 4: 834, 12: 1440}      # seeds whose reference plan meets the preconditions below


def _geom_scene(S):
    return commit_scene(GEOM_SEEDS[S], n=300, per_node=(0, 12), S=S, q=200, groups=5, fit_density=0.95, protected_share=0.2, flagged=0.05)


@pytest.mark.parametrize("S", [0, 1, 4, 12])
def test_plan_and_applied_state_do_not_depend_on_the_chunk_split(S, monkeypatch):
    """classifier counts when written, S = 0 / 1 / 4 / 12: at 5 nodes a chunk later entries 471 / 422 / 462 / 76 and rescans 3 / 1 / 1 / 2; as
    one chunk of 300 nodes rescans in 100 / 76 / 79 / 18 slots"""
    n = 300
    sc = _geom_scene(S)
    assert sc["nodes"].flags.any() and sc["protected"].any() and not sc["protected"].all()
    exp = _expect(sc, 8, True, True)
    c5, c1 = paths.classify(sc, exp["res"], 5), paths.classify(sc, exp["res"], n)
    print(f"\nS={S}: {paths.summary(c5)}\n      {paths.summary(c1)}")
    assert c5["later"] > 0 and c5["rescans"] > 0
    assert c1["nchunks"] == 1 and c1["rescans"] > 0 and c1["rescans_max"] == 1
    first = None
    for v in (1, 3, 4, 5, 64, n):
        monkeypatch.setenv(HOOK, str(v))
        where = f"S={S} {HOOK}={v}"
        with _ctx(sc) as ctx:
            got, dt = _commit(ctx, sc, 8, True, True)
            _compare(got, exp["res"], where)
            _compare_state(ctx, exp, where)
            blob = [got[f].tobytes() for f in FIELDS] + [a.tobytes() for a in _state(ctx)]
        print(f"  {where}: device call {dt * 1e3:.1f} ms")
        first = first or blob
        assert blob == first, where + ": outputs or applied state differ from the one-node-a-chunk answer"


def test_preempt_run_does_not_depend_on_the_chunk_split(monkeypatch):
    """bs_preempt_run keeps no records, but its merge over the chunks (k_preempt_pick) sees 300, 100, 75, 60, 5 and 1 of them"""
    S, n = 4, 300
    sc = _geom_scene(S)
    want = pr.preempt_np(pr.Prep(sc["nodes"], sc["bound"], S), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], 8)
    assert np.any(want["n_victims"] > 0) and np.any(want["node"] < 0) and np.unique(want["node"]).size > 20
    for v in (1, 3, 4, 5, 64, n):
        monkeypatch.setenv(HOOK, str(v))
        with _ctx(sc) as ctx:
            got = ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=8)
        _compare(got, want, f"bs_preempt_run {HOOK}={v}")


# ---- c. the rescan list's spill: a ladder with a closed-form answer
def ladder_scene(S, N, q):
    """N identical empty nodes (cpu 1000 allocatable, nothing requested, no scalar keys, no flags, nothing bound), q preemptors of class 0
    that each ask for cpu 1000, fit all ones: a node holds exactly one nominee"""
    L = 4 + S
    al = np.zeros((L, N), np.int64)
    al[0], al[3] = 1000, 110
    nodes = soa.Nodes(al, np.zeros((L, N), np.int64), np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint8))
    req = np.zeros((L, q), np.int64)
    req[0] = 1000
    pods = soa.Pods(np.full(q, soa.POD_NOT_GROUPED, np.int32), req, np.zeros(q, np.uint32), np.zeros(q, np.uint32), np.zeros(q, np.uint64),
                    np.zeros(q, np.uint8))
    rng = np.random.default_rng(N + q)
    return dict(nodes=nodes, fit=soa.FitMasks.from_bool(np.ones((1, N), bool)), pods=pods, bound=soa.Bound.empty(0, L), S=S,
                protected=np.zeros(1, np.uint8), pod_index=rng.permutation(q).astype(np.uint32),
                priority=rng.choice([0, 7, 1000], size=q).astype(np.int32), groups=1)


# (S, nodes, preemptors, hook, the last chunk is rescanned)
LADDERS = [(12, 1400, 1300, 5, False), (0, 2700, 2600, 5, False), (12, 1403, 1300, 5, False), (12, 1825, 1828, 7, True)]


@pytest.mark.parametrize("S,N,q,hook,last", LADDERS)
def test_rescan_list_spills_on_a_ladder_with_a_closed_form_answer(S, N, q, hook, last, monkeypatch):
    """Slot s (in slot order) takes node s and sees N - s candidates; a chunk whose four recorded nodes are taken is rescanned by every
    later slot, so late slots rescan more chunks than the list holds (classifier when written: at most 260, 520, 260, 261 in a slot, against
    256, 512, 256, 256 entries) and the threads that could not list a chunk walk it themselves.
    The third case has a partial last chunk (1403 mod 5 = 3).  A partial chunk of a 5-node split holds at most four nodes and is therefore
    never rescanned, so the rescan walk's k >= N is not crossed there; the fourth case crosses it: 7 nodes a chunk, a last chunk of 5 nodes
    (1825 mod 7), and more preemptors than nodes, so that the last chunk's record goes dirty, it is rescanned past the node list's end, and
    the last three slots find no node at all."""
    sc = ladder_scene(S, N, q)
    t0 = time.perf_counter()
    exp = _expect(sc, 4, True, True)
    cl = paths.classify(sc, exp["res"], hook, detail=True)
    t_ref = time.perf_counter() - t0
    print(f"\nladder S={S} N={N} q={q} {HOOK}={hook}: {paths.summary(cl)}")
    assert cl["rescans_max"] > pc_threads(S), "the scene does not fill the rescan list"
    assert (N % hook != 0) == (N in (1403, 1825))
    assert any(cl["nchunks"] - 1 in x["rescanned"] for x in cl["slots"]) == last
    order, s = pc.slot_order(sc["priority"]), np.arange(q)
    node, ncand = np.where(s < N, s, -1), np.maximum(N - s, 0)
    monkeypatch.setenv(HOOK, str(hook))
    where = f"ladder S={S} N={N} q={q}"
    with _ctx(sc) as ctx:
        got, t_plan = _commit(ctx, sc, 4)
        for res, who in ((exp["res"], "the reference"), (got, "the device")):
            assert np.array_equal(res["node"][order], node), f"{where}: {who} leaves the closed form (node)"
            assert np.array_equal(res["n_candidates"][order], ncand), f"{where}: {who} leaves the closed form (n_candidates)"
            assert not res["n_victims"].any() and not res["victims"].any()
        _compare(got, exp["res"], where + " plan")
        got, t_apply = _commit(ctx, sc, 4, True, True)
        _compare(got, exp["res"], where + " apply+assume")
        _compare_state(ctx, exp, where + " apply+assume")
        req, _ = ctx.read_node_requests()
        assert np.array_equal(req[0], np.where(np.arange(N) < q, 1000, 0)) and np.array_equal(req[3], (np.arange(N) < q).astype(np.int64))
    print(f"oracle + classifier {t_ref:.2f} s; device calls: plan {t_plan * 1e3:.1f} ms, apply+assume {t_apply * 1e3:.1f} ms")


# ---- d. PDB bits with chunks of several nodes: (S, nodes, bound pods per node, preemptors, groups, bit share, seeds)
PDB_SMALL = [(1, 60, (0, 12), 70, 6, 0.5, (5221, 5101)), (12, 120, (2, 14), 65, 6, 0.5, (5212, 5102))]
PDB_FIELDS = pp.FIELDS


@pytest.mark.parametrize("S,n,per,q,groups,share,seeds", PDB_SMALL)
def test_pdb_bits_under_forced_chunk_splits(S, n, per, q, groups, share, seeds, monkeypatch):
    """Two seeds a case, the preconditions hold over the pair (as tests/test_gpu_preempt_pdb.py holds its conditions over a scene set): with
    the violation count leading the key, at 5 nodes a chunk later entries (S = 1: 52 and 18, S = 12: 9 and 3) and a rescan (first seed: 1);
    as one chunk rescans (S = 1: second seed 10, S = 12: second seed 3); records of four victim-free nodes in front of a candidate
    node with violating pods; the bits changed the answer of every scene."""
    later5 = rescans5 = rescans1 = early = 0
    for seed in seeds:
        sc, bits = pp.pdb_scene(seed, n, per, S, q, groups, share)
        exp = _expect(sc, 8, True, True, bits)
        plain = _expect(sc, 8, bits=np.zeros_like(bits))
        assert "changed" in pp.effects(sc, exp["res"], plain["res"], bits), f"seed {seed}: the bits change nothing"
        c5, c1 = paths.classify(sc, exp["res"], 5, bits=bits), paths.classify(sc, exp["res"], n, bits=bits)
        print(f"\nS={S} n={n} seed={seed}: {paths.summary(c5)}\n      {paths.summary(c1)}")
        later5 += c5["later"]
        rescans5 += c5["rescans"]
        rescans1 += c1["rescans"]
        early += c5["early_exit_before_violating"] + c1["early_exit_before_violating"]
        first = None
        for v in (1, 5, n):
            monkeypatch.setenv(HOOK, str(v))
            where = f"pdb S={S} n={n} seed={seed} {HOOK}={v}"
            with _ctx(sc, bits) as ctx:
                got, _ = _commit(ctx, sc, 8)
                _compare(got, exp["res"], where + " plan", PDB_FIELDS)
                got, _ = _commit(ctx, sc, 8, True, True)
                _compare(got, exp["res"], where + " apply+assume", PDB_FIELDS)
                _compare_state(ctx, exp, where)
                blob = [got[f].tobytes() for f in PDB_FIELDS] + [a.tobytes() for a in _state(ctx)]
            first = first or blob
            assert blob == first, where
    assert later5 > 0 and rescans5 > 0 and rescans1 > 0 and early > 0, (later5, rescans5, rescans1, early)


def test_pdb_bits_shipped_geometry_large_queue(monkeypatch):
    """(S, n, per, q, groups, share) = (4, 400, (1, 6), 4096, 6, 0.4), 7 nodes a chunk as shipped.  q stays at 4096 (a smaller queue means
    more chunks of fewer nodes, down to four and less, which never rescan); the references (with bits, and without for the effects) and the
    classifier take a few seconds together.  Classifier when written: later entries 1475, rescans 429 (13 in one slot),
    81 records of four victim-free nodes in front of a candidate node with violating pods, n_candidates corrected in 3436 slots."""
    monkeypatch.delenv(HOOK, raising=False)
    S, n, q = 4, 400, 4096
    sc, bits = pp.pdb_scene(5100, n, (1, 6), S, q, 6, 0.4)
    t0 = time.perf_counter()
    cn = paths.geometry(n, count=q)[2]
    assert cn == 7
    exp = _expect(sc, 8, True, True, bits)
    plain = _expect(sc, 8, bits=np.zeros_like(bits))
    eff = pp.effects(sc, exp["res"], plain["res"], bits)
    cl = paths.classify(sc, exp["res"], cn, bits=bits)
    t_ref = time.perf_counter() - t0
    print(f"\npdb S={S} n={n} q={q}: {paths.summary(cl)}; effects {sorted(eff)}")
    assert {"changed", "node_differs", "violations_on_chosen"} <= eff
    assert cl["later"] > 0 and cl["rescans"] > 0 and cl["rescans_max"] >= 2 and cl["early_exit_before_violating"] > 0 and cl["ncand_corrected"] > 0
    with _ctx(sc, bits) as ctx:
        got, t_plan = _commit(ctx, sc, 8)
        _compare(got, exp["res"], "pdb large queue plan", PDB_FIELDS)
        got, t_apply = _commit(ctx, sc, 8, True, True)
        _compare(got, exp["res"], "pdb large queue apply+assume", PDB_FIELDS)
        _compare_state(ctx, exp, "pdb large queue")
    print(f"oracle + classifier {t_ref:.2f} s; device calls: plan {t_plan * 1e3:.1f} ms, apply+assume {t_apply * 1e3:.1f} ms")
