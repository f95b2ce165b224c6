"""GPU tests of bs_preempt_commit_gang / bs_preempt_gang_read (csrc/bs_preempt_commit_gang.hpp: k_gang_resolve, the quorum of each gang's run
and the rollback).  Everything is compared bit for bit with the defining-property restatement of tests/preempt_gang_ref.py (itself held
against the object-level one and hand known answers by tests/test_preempt_gang_cpu.py): every field of preempt_commit's dict,
n_pdb_violations, slot_voided, group_placed, and after APPLY / ASSUME the node requests, present bits, bs_bound_read and bs_bound_count.

Every scene test first asserts on the CPU classifier (tests/preempt_gang_paths.py) that its scene takes the path it is about; the seeds
were picked on the CPU for that.  The shapes are the smallest at which the rollback can go wrong, none is the workload's size."""
import ctypes as C
import importlib

import numpy as np
import pytest

import preempt_gang_paths as gp
import preempt_gang_scenes as gs
import preempt_pdb_ref as pp
from preempt_scenes import groups_for

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa = bsa.soa
HOOK = "BS_TEST_PC_CHUNK_NODES"
MODES = ((False, False), (True, False), (True, True))


def _ctx(sc):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    if sc.get("violating") is not None:
        ctx.bound_pdb_set(sc["violating"])
    return ctx


def _state(ctx) -> dict:
    req, pres = ctx.read_node_requests()
    ids, nodes = ctx.read_bound()
    assert ctx.bound_count() == ids.size
    return dict(req=req, pres=pres, bound_id=ids, bound_node=nodes)


def _gang(ctx, sc, cap, apply=False, assume=False, flat=False) -> dict:
    res = ctx.preempt_commit_gang(sc["pod_index"], sc["priority"], sc["protected"], sc["need"], victim_cap=cap, apply=apply, assume=assume, flat=flat)
    got = dict(res=res, slot_voided=res["slot_voided"], group_placed=res["group_placed"])
    got.update(_state(ctx))
    return got


def _compare(got, exp, where):
    for f in pp.FIELDS:
        a, b = got["res"][f], exp["res"][f]
        if not np.array_equal(a, b):
            bad = np.nonzero(np.any((a != b).reshape(len(a), -1), axis=1))[0]
            i = int(bad[0])
            pytest.fail(f"{where}: {f} differs at preemptor {i} of {len(bad)} bad: got {a[i]} expected {b[i]} (node {got['res']['node'][i]} vs "
                        f"{exp['res']['node'][i]}, voided {got['slot_voided'][i]} vs {exp['slot_voided'][i]})")
    for f in ("slot_voided", "group_placed") + gs.STATE:
        assert np.array_equal(got[f], exp[f]), f"{where}: {f}: {np.asarray(got[f]).tolist()[:40]} vs {np.asarray(exp[f]).tolist()[:40]}"


def _check(sc, cap, modes=MODES, where=""):
    for apply, assume in modes:
        exp = gs.expect(sc, cap, apply, assume)
        with _ctx(sc) as ctx:
            got = _gang(ctx, sc, cap, apply, assume)
        _compare(got, exp, f"{where} cap={cap} apply={apply} assume={assume}")
        assert not np.any(got["res"]["n_pdb_violations"][got["slot_voided"] != 0])
    return exp


def _paths(sc, cap, *want):
    c = gp.classify(sc, cap)
    for k in ("voided_placed", "standing") + want:
        assert c[k] > 0, f"the scene does not take the path {k}: {gp.summary(c)}"
    return c


# ---- 1. the hand known answers
def test_hand_known_answers_on_device():
    for sc in gs.gang_kats():
        s = gs.kat_gang_scene(sc)
        with _ctx(s) as ctx:
            got = _gang(ctx, s, s["cap"], s["apply"], s["assume"])
        gs.check_gang_kat(got, sc, f"device {sc['name']}")


# ---- 2. a voided run whose two slots chose the same node: the bit words restored last slot first, two nominees in dn
@pytest.mark.parametrize("S,seed", [(0, 400), (1, 400), (4, 400), (12, 2229)])
def test_voided_run_with_two_slots_on_one_node(S, seed):
    sc = gs.gang_scene(seed, n=4, per_node=(6, 12), S=S, q=16, groups=3, fit_density=1.0, flagged=0.0)
    _paths(sc, 4, "same_node")
    _check(sc, 4, where=f"same node S={S}")


# ---- 3. a voided run's victim evicted again later, a later slot on a node the voided run dirtied (zero deltas; n_candidates)
@pytest.mark.parametrize("S", [0, 4])
def test_later_slots_reuse_what_a_voided_run_touched(S):
    sc = gs.gang_scene(205, n=6, per_node=(3, 9), S=S, q=24, groups=5)
    _paths(sc, 4, "revictim", "dirty_reuse")
    _check(sc, 4, where=f"reuse S={S}")


# ---- 4. victim_cap 0 and 1 with voided slots of three or more victims: the undo does not read the truncated list
@pytest.mark.parametrize("cap", [0, 1])
def test_undo_does_not_depend_on_victim_cap(cap):
    sc = gs.gang_scene(513, n=6, per_node=(8, 16), S=1, q=20, groups=4, fit_density=1.0)
    _paths(sc, cap, "big_voided", "over_cap")
    _check(sc, cap, where="cap")



# ---- 4b. a context with no groups: no gang column has a requirement, the protected column is clamped to one byte
@pytest.mark.parametrize("cap", [0, 6])
def test_a_context_with_no_groups(cap):
    from preempt_scenes import ungrouped_scene
    sc = ungrouped_scene(gs.gang_scene(8600, n=70, per_node=(2, 9), S=2, q=65, groups=4, p=70))
    sc["need"] = np.zeros(0, np.uint32)
    exp = _check(sc, cap, modes=((True, True),), where="no groups")
    assert np.any(exp["res"]["n_victims"] > 0) and not exp["slot_voided"].any() and exp["group_placed"].size == 0


# ---- 5. voided and standing runs on nodes with PDB-violating entries (two-pass reprieve)
@pytest.mark.parametrize("S", [0, 4])
def test_pdb_violating_entries_in_voided_and_standing_runs(S):
    sc = gs.gang_scene(403, n=8, per_node=(4, 10), S=S, q=24, groups=5, share=0.5)
    _paths(sc, 4, "pdb_voided", "pdb_standing")
    exp = _check(sc, 4, where=f"pdb S={S}")
    assert np.any(exp["res"]["n_pdb_violations"] > 0)


# ---- 6. placement and size of runs, lists of 130 slots
def test_placement_and_size_of_runs():
    seen = {}
    for seed in (500, 505, 506):
        sc = gs.gang_scene(seed, n=40, per_node=(2, 9), S=1, q=130, groups=14, p=260)
        for k, v in _paths(sc, 4).items():
            seen[k] = seen.get(k, 0) + v
        _check(sc, 4, modes=((True, True),), where=f"placement seed {seed}")
    for k in ("run_at_end", "back_to_back", "run_of_one", "need_eq_placed", "need_gt_len", "ungrouped_between"):
        assert seen[k] > 0, (k, seen)


# ---- 7. chunks holding several nodes: the same answer for every split
def test_answers_do_not_depend_on_the_chunk_split(monkeypatch):
    n = 65
    sc = gs.gang_scene(600, n=n, per_node=(2, 9), S=4, q=130, groups=9)
    _paths(sc, 4, "dirty_reuse")
    exp = gs.expect(sc, 4, True, True)
    for v in (1, 3, 64, n):
        monkeypatch.setenv(HOOK, str(v))
        with _ctx(sc) as ctx:
            got = _gang(ctx, sc, 4, True, True)
        _compare(got, exp, f"{HOOK}={v}")


# ---- 8. random scenes; the defining property on the device: a twin context runs bs_preempt_commit on the surviving preemptors
@pytest.mark.parametrize("S,n,per,q,seed", [(0, 64, (2, 9), 130, 700), (1, 3, (63, 65), 65, 1098), (4, 65, (30, 60), 130, 704), (12, 64, (2, 9), 130, 712)])
def test_random_scenes_and_the_defining_property_on_a_twin_context(S, n, per, q, seed):
    sc = gs.gang_scene(seed, n=n, per_node=per, S=S, q=q, groups=9)
    _paths(sc, 6)
    for apply, assume in MODES:
        where = f"S={S} n={n} q={q} apply={apply} assume={assume}"
        exp = gs.expect(sc, 6, apply, assume)
        with _ctx(sc) as ctx:
            got = _gang(ctx, sc, 6, apply, assume)
        _compare(got, exp, where)
        keep = np.array(exp["keep"], np.int64)
        assert 0 < keep.size < q
        with _ctx(sc) as twin:
            plain = twin.preempt_commit(sc["pod_index"][keep], sc["priority"][keep], sc["protected"], victim_cap=6, apply=apply, assume=assume)
            tstate = _state(twin)
        for f in pp.FIELDS:
            assert np.array_equal(got["res"][f][keep], plain[f]), f"{where}: twin {f}"
        for f in gs.STATE:
            assert np.array_equal(got[f], tstate[f]), f"{where}: twin state {f}"


# ---- 9. all needs 0 equals bs_preempt_commit on a twin context
@pytest.mark.parametrize("S", [0, 4, 12])
def test_all_needs_zero_is_bs_preempt_commit(S):
    sc = gs.gang_scene(700 + S, n=64, per_node=(2, 9), S=S, q=130, groups=9, share=0.2)
    sc["need"][:] = 0
    for apply, assume in MODES:
        with _ctx(sc) as ctx, _ctx(sc) as twin:
            got = _gang(ctx, sc, 6, apply, assume, flat=apply and not assume)
            plain = twin.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=6, apply=apply, assume=assume)
            tstate = _state(twin)
        assert np.any(plain["n_victims"] > 0)
        for f in pp.FIELDS:
            assert np.array_equal(got["res"][f], plain[f]), f
        for f in gs.STATE:
            assert np.array_equal(got[f], tstate[f]), f
        assert not got["slot_voided"].any() and not got["group_placed"].any()


# ---- 10. error codes, each with the state unchanged
def test_error_codes_leave_the_state_alone():
    sc = gs.gang_scene(205, n=6, per_node=(3, 9), S=0, q=24, groups=5)
    B = bsa.BsError
    grp = np.asarray(sc["pods"].group)[sc["pod_index"]]
    with _ctx(sc) as ctx:
        before = _state(ctx)

        def unchanged():
            after = _state(ctx)
            for f in gs.STATE:
                assert np.array_equal(before[f], after[f]), f

        def refused(status, pod_index, priority, need, **kw):
            with pytest.raises(B) as e:
                ctx.preempt_commit_gang(pod_index, priority, sc["protected"], need, **kw)
            assert e.value.status == status, (e.value, kw)
            unchanged()

        with pytest.raises(B) as e:                                  # nothing to read yet
            ctx._chk(ctx._lib.bs_preempt_gang_read(ctx._h, 0, None, 0, None), "bs_preempt_gang_read")
        assert e.value.status == -4
        # a group in two runs: its members at two priorities with another preemptor's priority in between
        g = int(grp[grp >= 0][0])
        m, other = np.nonzero(grp == g)[0], np.nonzero(grp != g)[0]
        prio = sc["priority"].copy()
        prio[m[0]], prio[other[0]] = 9000, 8000
        prio[m[1:]] = 7000
        need = np.zeros_like(sc["need"])
        need[g] = 1
        refused(-1, sc["pod_index"], prio, need, apply=True)
        refused(-1, sc["pod_index"], sc["priority"], None, apply=True)                   # NULL need with g > 0
        refused(-1, [3, 5, 3], [9, 8, 7], sc["need"], apply=True)                        # whatever bs_preempt_commit refuses
        refused(-1, sc["pod_index"], sc["priority"], sc["need"], apply=False, assume=True)
        refused(-1, [10 ** 6], [5], sc["need"], apply=True)
        refused(-1, [0], [5], sc["need"], apply=True, stages=soa.STAGE_FILTER)
        # the getter follows the last preemption call
        res = ctx.preempt_commit_gang(sc["pod_index"], sc["priority"], sc["protected"], sc["need"])
        unchanged()
        q, g_count = len(sc["pod_index"]), sc["groups"]
        voided, placed = np.zeros(q, np.uint8), np.zeros(g_count, np.uint32)
        u8, u32 = voided.ctypes.data_as(C.POINTER(C.c_uint8)), placed.ctypes.data_as(C.POINTER(C.c_uint32))
        read = ctx._lib.bs_preempt_gang_read
        assert read(ctx._h, q, u8, g_count, u32) == 0 and np.array_equal(voided, res["slot_voided"]) and np.array_equal(placed, res["group_placed"])
        assert read(ctx._h, q, None, g_count, None) == 0
        assert read(ctx._h, q + 1, u8, g_count, u32) == -1 and read(ctx._h, q, u8, g_count + 1, u32) == -1
        ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"])
        assert read(ctx._h, q, u8, g_count, u32) == -4               # BS_ERR_STATE after a plain bs_preempt_commit
        ctx.preempt_commit_gang(sc["pod_index"], sc["priority"], sc["protected"], sc["need"])
        ctx.preempt(sc["pod_index"], sc["priority"], sc["protected"])
        assert read(ctx._h, q, u8, g_count, u32) == -4               # ... and after bs_preempt_run
        ctx.set_shard(0, 2)
        refused(-4, sc["pod_index"], sc["priority"], sc["need"], apply=True)             # single-rank only
        ctx.set_shard(0, 1)

