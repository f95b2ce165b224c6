"""GPU tests of BS_PREEMPT_CLEAR_LOWER (include/bsched.h, rule C; csrc/bs_preempt_clear.hpp: k_nc_resolve<S>; bs_nominated.hpp: k_nc_list;
bs_preempt_cleared_read).

Three kinds of check.  The hand known answers (tests/golden/preempt_clear_hand_kats.json) on the device.  tests/preempt_clear_ref.py's
threshold statement (held against the object statement by tests/test_preempt_clear_cpu.py) in every flag mode.  And twin contexts with no
model in between: one flagged call against single-slot flag-less calls with a host-side removal in between, and a flagged call that can
clear nothing against the flag-less call.  The shapes are the smallest at which each mechanism can go wrong: 40 nodes and 24 preemptors
put several takers on one node, chunks of 5 and of 40 nodes reach the record fallback and the rescan, 1023 / 1024 / 1025 rows are
k_nc_list's window edge."""
import copy
import importlib

import numpy as np
import pytest

import nominated_ref as nr
import preempt_clear_ref as cr
import preempt_commit_ref as pc
import preempt_gang_scenes as gs
import preempt_pdb_ref as pp
from preempt_scenes import groups_for, kat_scene
from test_preempt_clear_cpu import check_kat, kat_rows, kats

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, capi = bsa.soa, bsa.capi
HOOK = "BS_TEST_PC_CHUNK_NODES"
INVALID, STATE_ERR = -1, -4
CAP = 8
MODES = ("plan", "apply", "assume", "nominate")           # flags 0, APPLY, APPLY|ASSUME, APPLY|NOMINATE — each with CLEAR_LOWER


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _ctx(sc, rows=None):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"], sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    if sc.get("violating") is not None:
        ctx.bound_pdb_set(sc["violating"])
    if rows is not None:
        ctx.nominated_load(rows["node"], rows["priority"], rows["req"], rows["req_present"])
    return ctx


def _call(ctx, sc, mode, clear=True, pick=None) -> dict:
    pi, pr_ = (sc["pod_index"], sc["priority"]) if pick is None else (sc["pod_index"][pick], sc["priority"][pick])
    kw = dict(victim_cap=CAP, apply=mode != "plan", assume=mode == "assume", nominate=mode == "nominate", clear_lower=clear)
    if sc.get("need") is None:
        return ctx.preempt_commit(pi, pr_, sc["protected"], **kw)
    return ctx.preempt_commit_gang(pi, pr_, sc["protected"], sc["need"], **kw)


def _expect(sc, rows, mode) -> dict:
    prep = pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], sc["violating"])
    a = (prep, sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"], sc["protected"])
    if sc.get("need") is None:
        return cr.commit_clear_np(*a, CAP, rows, mode != "plan", mode == "assume")
    return cr.gang_clear_np(*a, sc["need"], CAP, rows, mode != "plan", mode == "assume")


def _bare(sc, rows) -> dict:
    prep = pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], sc["violating"])
    a = (prep, sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"], sc["protected"])
    return (nr.commit_nom_np(*a, CAP, rows) if sc.get("need") is None else nr.gang_nom_np(*a, sc["need"], CAP, rows))["res"]


def _same(got, exp, where, fields=pp.FIELDS):
    for f in fields:
        if f in exp and not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(np.any((np.asarray(got[f]) != np.asarray(exp[f])).reshape(len(got[f]), -1), axis=1))[0]
            i = int(bad[0])
            pytest.fail(f"{where}: {f} differs at {i} of {len(bad)} bad: got {got[f][i]} expected {exp[f][i]}")


def _same_cleared(got, exp, where):
    for f in cr.CLEARED:
        assert np.array_equal(got[f], exp[f]), f"{where}: cleared {f}: {got[f].tolist()[:16]} vs {exp[f].tolist()[:16]}"


def _state(ctx) -> dict:
    req, pres = ctx.read_node_requests()
    ids, nodes = ctx.read_bound()
    return dict(req=req, pres=pres, bound_id=ids, bound_node=nodes)


def _everything(ctx) -> dict:
    """what the twin tests hold byte-equal: bs_bound_dump, bs_nodes_read, bs_bound_read and bs_nominated_read"""
    out = {"dump." + k: v for k, v in ctx.bound_dump().items()}
    out.update({"state." + k: v for k, v in _state(ctx).items()})
    try:
        out.update({"nom." + k: v for k, v in ctx.nominated_read().items()})
    except capi.BsError:
        pass
    return out


def _equal_everything(a, b, where):
    assert a.keys() == b.keys(), where
    for f in a:
        assert np.array_equal(a[f], b[f]), f"{where}: {f}"


def _model_table(sc, rows):
    t = nr.NomTable(sc["S"])
    t.load(sc["nodes"].n, rows["node"], rows["priority"], rows["req"], rows["req_present"])
    return t


def _read_equal(ctx, exp: dict, where):
    got = ctx.nominated_read()
    assert ctx.nominated_count() == exp["id"].size, where
    for f in exp:
        assert np.array_equal(got[f], exp[f]), f"{where}: {f}: {got[f].tolist()[:24]} vs {exp[f].tolist()[:24]}"


def _refused(status, fn, *a, **kw):
    with pytest.raises(capi.BsError) as e:
        fn(*a, **kw)
    assert e.value.status == status, str(e.value)


def _check_against_ref(sc, rows, mode, where):
    """one flagged call on a fresh context against the threshold statement: answers, resident state, gang columns, the report, the table"""
    exp = _expect(sc, rows, mode)
    model = _model_table(sc, rows)
    ids = cr.table_after(model, exp, sc["pod_index"], sc["priority"], sc["pods"], mode != "plan", mode == "nominate")
    with _ctx(sc, rows) as ctx:
        got = _call(ctx, sc, mode)
        _same(got, exp["res"], where)
        _same(_state(ctx), exp, where + " state", gs.STATE)
        if sc.get("need") is not None:
            _same(got, exp, where, ("slot_voided", "group_placed"))
        _same_cleared(got["cleared"], exp["cleared"], where)
        if mode == "nominate":
            assert np.array_equal(got["nominated_id"], ids), where
        _read_equal(ctx, model.read(), where + ": the table afterwards")
        assert ctx.nominated_ids() == model.ids
    return got, exp


def _widen(k: dict, S: int) -> dict:
    """a hand vector (written for S = 0) on a context with S scalar lanes nobody uses"""
    k = copy.deepcopy(k)
    for part, f in (("nodes", "alloc"), ("nodes", "req"), ("pods", "req"), ("bound", "req"), ("rows", "req")):
        k[part][f] = k[part][f] + [[0] * len(k[part][f][0]) for _ in range(S)]
    k["S"] = S
    return k


# ---- 1. the hand known answers (the two rollback vectors and bs_preempt_gang_read among them) ------------------------------------------
@pytest.mark.parametrize("S", [0, 2])
def test_hand_known_answers_on_device(S):
    for k0 in kats():
        k = _widen(k0, S)
        s = kat_scene(k)
        s["violating"] = None
        s["need"] = np.array(k["need"], np.uint32) if k["call"] == "gang" else None
        with _ctx(s, kat_rows(k).read()) as ctx:
            got = _call(ctx, s, k["mode"])
            plan = dict(res=got, cleared=got["cleared"], slot_voided=got.get("slot_voided"), group_placed=got.get("group_placed"))
            table = ctx.nominated_read()
            check_kat(plan, table["id"], k, f"{k['name']} S={S}")
            for f, v in k.get("expect_table", {}).items():
                assert table[f].tolist() == v, f"{k['name']}: table {f}"
            if "expect_nodes_without_flag" in k:
                with _ctx(s, kat_rows(k).read()) as twin:
                    assert _call(twin, s, "plan", clear=False)["node"].tolist() == k["expect_nodes_without_flag"], k["name"]


# ---- 2. against the reference ------------------------------------------------------------------------------------------------------------
SEED = 308            # picked on the CPU: at 40 nodes and 24 preemptors, for S in {0, 2, 12}, commit and gang, the flag changes an answer, at
                      # least 3 rows are cleared, a gang run is voided, and two taken nodes share a chunk of 5 (each test asserts what it needs)


def _scene(seed, S, gang, n=40, q=24):
    sc = cr.clear_scene(seed, gang, n=n, q=q, S=S)
    return sc, cr.clear_rows_for(sc, seed, density=1.0, per_node=(1, 3), heavy=0.5)


@pytest.mark.parametrize("S", [0, 2, 12])
@pytest.mark.parametrize("gang", [False, True], ids=["commit", "gang"])
def test_every_flag_mode_against_the_reference(gang, S):
    sc, rows = _scene(SEED, S, gang)
    for mode in MODES:
        got, exp = _check_against_ref(sc, rows, mode, f"{'gang' if gang else 'commit'} S={S} {mode}")
    assert exp["cleared"]["id"].size >= 3, "the scene clears next to nothing"
    assert nr.changed(exp["res"], _bare(sc, rows)), "the flag changes no answer of this scene"
    if gang:
        assert np.any(exp["slot_voided"] != 0), "no run of this scene is voided"


@pytest.mark.parametrize("cn", [5, 40])
def test_chunks_of_several_nodes_meet_cleared_rows(cn, monkeypatch):
    """the chunk-size hook of tests/test_gpu_preempt_commit_chunks.py: with 5 nodes a chunk a taken node leaves its chunk's record to the
    later entries, with all 40 nodes in one chunk the chunk is rescanned; in both a node some slot stands on (dirty, threshold raised)
    shares its chunk with nodes that hold rows"""
    monkeypatch.setenv(HOOK, str(cn))
    for gang in (False, True):
        sc, rows = _scene(SEED, 2, gang)
        got, exp = _check_against_ref(sc, rows, "apply", f"{HOOK}={cn} gang={gang}")
        taken = np.unique(exp["res"]["node"][exp["res"]["node"] >= 0])
        assert any(a != b and a // cn == b // cn for a in taken for b in taken), "no two taken nodes share a chunk"
        assert exp["cleared"]["id"].size and nr.changed(exp["res"], _bare(sc, rows))


# ---- 3. twin contexts, existing calls only -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 2])
def test_one_flagged_call_equals_single_slot_calls_with_a_removal_in_between(S):
    """bs_preempt_commit(APPLY | NOMINATE | CLEAR_LOWER), preemptors passed in slot order, against q flag-less single-slot
    bs_preempt_commit(APPLY | NOMINATE) calls on a twin, with bs_nominated_apply removing the rows below the preemptor's priority on the
    node it took in between: equal answers (n_candidates included), byte-equal bs_bound_dump, bs_nodes_read and bs_nominated_read"""
    sc, rows = _scene(340 + S, S, False)
    o = pc.slot_order(sc["priority"])
    sc["pod_index"], sc["priority"] = sc["pod_index"][o], sc["priority"][o]
    q = len(o)
    with _ctx(sc, rows) as ctx, _ctx(sc, rows) as twin:
        got = _call(ctx, sc, "nominate")
        removed = []
        for i in range(q):
            one = _call(twin, sc, "nominate", clear=False, pick=[i])
            for f in pp.FIELDS + ("nominated_id",):
                assert np.array_equal(one[f][0], got[f][i]), f"slot {i}: {f}: {one[f][0]} vs {got[f][i]}"
            k = int(one["node"][0])
            if k >= 0:
                t = twin.nominated_read()
                lower = t["id"][(t["node"] == k) & (t["priority"] < sc["priority"][i])]
                removed += [int(x) for x in lower]
                if lower.size:
                    twin.nominated_apply(lower)
        assert sorted(removed) == got["cleared"]["id"].tolist() and len(removed) >= 3, "the removals are the report"
        _equal_everything(_everything(ctx), _everything(twin), f"S={S}")
        assert ctx.nominated_ids() == twin.nominated_ids()


@pytest.mark.parametrize("gang", [False, True], ids=["commit", "gang"])
def test_the_flag_with_no_qualifying_row_is_the_flagless_call(gang):
    """rows at or above the highest preemptor priority (k_nc_resolve runs, nothing can be cleared), an empty table and no table (today's
    kernels run): results and resident state are byte-equal to the call without the flag, and the report is empty"""
    sc, rows = _scene(360 + gang, 2, gang)
    high = dict(rows, priority=np.maximum(rows["priority"], int(sc["priority"].max())).astype(np.int32))
    empty = {k: (v[:, :0] if k == "req" else v[:0]) for k, v in rows.items()}
    for name, r in (("rows that never qualify", high), ("an empty table", empty), ("no table", None)):
        for mode in ("plan", "apply"):
            with _ctx(sc, r) as ctx, _ctx(sc, r) as twin:
                got, want = _call(ctx, sc, mode), _call(twin, sc, mode, clear=False)
                _same(got, want, f"{name} {mode}", pp.FIELDS + (("slot_voided", "group_placed") if gang else ()))
                _equal_everything(_everything(ctx), _everything(twin), f"{name} {mode}")
                assert got["cleared"]["id"].size == 0 and ctx.preempt_cleared_read(0)["n"] == 0


# ---- 4. APPLY: the table, dead ids, the list kernel's window edge --------------------------------------------------------------------------
def test_a_cleared_id_is_dead_after_apply_and_alive_without():
    sc, rows = _scene(380, 2, False)
    with _ctx(sc, rows) as ctx:
        got = _call(ctx, sc, "plan")
        gone = got["cleared"]["id"]
        assert gone.size >= 2
        _read_equal(ctx, rows, "without APPLY nothing resident changes")
        got2 = _call(ctx, sc, "apply")
        assert np.array_equal(got2["cleared"]["id"], gone)
        _refused(INVALID, ctx.nominated_apply, gone[:1])                          # dead, as after bs_nominated_apply
        _refused(INVALID, ctx.nominated_apply, [int(gone[-1]), int(rows["id"][~np.isin(rows["id"], gone)][0])])
        assert ctx.nominated_count() == rows["id"].size - gone.size and ctx.nominated_ids() == rows["id"].size


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_clears_on_both_sides_of_the_list_kernels_window_edge(m):
    """k_nc_list walks the rows in windows of 1024 with a running base: tables of 1023, 1024 and 1025 rows whose first row, last row and
    the rows around index 1023 sit on a taken node below every preemptor's priority, among many other cleared rows"""
    sc = cr.clear_scene(400, False, n=24, q=12, S=1)
    rng = np.random.default_rng(m)
    src = rng.integers(0, sc["pods"].p, size=m)
    req = sc["pods"].req[:5, src].astype(np.int64).copy()
    req[:3] //= 64                                                              # light rows: the plan keeps several takers
    lo, hi = int(sc["priority"].min()), int(sc["priority"].max())
    node, prio = rng.integers(0, 24, size=m), rng.integers(lo - 1, hi + 1, size=m)
    t = nr.NomTable(1)
    t.load(24, node, prio, req, sc["pods"].req_present[src])
    first = cr.commit_clear_np(pp.PdbPrep(sc["nodes"], sc["bound"], 1, sc["violating"]), sc["fit"], sc["pods"], sc["bound"], sc["pod_index"],
                               sc["priority"], sc["protected"], CAP, t.read())
    k = int(first["res"]["node"][first["res"]["node"] >= 0][0])                  # a node some preemptor takes
    edge = [e for e in (0, 1022, 1023, 1024, m - 1) if e < m]
    node[edge], prio[edge] = k, lo - 5                                          # below everyone: they count for nobody, the plan stays
    t.load(24, node, prio, req, sc["pods"].req_present[src])
    rows = t.read()
    got, exp = _check_against_ref(sc, rows, "apply", f"m={m}")
    assert set(edge) <= set(exp["cleared"]["id"].tolist()) and exp["cleared"]["id"].size > 100
    assert np.any(exp["cleared"]["id"] < 1023) and (m <= 1024 or np.any(exp["cleared"]["id"] >= 1024))


# ---- 5. refusals and the report's states ---------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing_and_the_reports_states():
    sc, rows = _scene(SEED, 2, True)
    pi, pr_, prot, need = sc["pod_index"], sc["priority"], sc["protected"], sc["need"]
    CL = soa.PREEMPT_CLEAR_LOWER
    with _ctx(sc, rows) as ctx:
        _refused(STATE_ERR, ctx.preempt_cleared_read, 0)                          # before any call
        ctx.preempt_commit(pi, pr_, prot, victim_cap=CAP)
        _refused(STATE_ERR, ctx.preempt_cleared_read, 0)                          # after a flag-less call
        got = _call(ctx, sc, "plan")
        n = got["cleared"]["id"].size
        assert n >= 3
        short = ctx.preempt_cleared_read(2)                                       # cap below n: the true count, the first rows
        assert short["n"] == n and all(np.array_equal(short[f], got["cleared"][f][:2]) for f in cr.CLEARED)
        assert ctx.preempt_cleared_read(0)["n"] == n                              # NULL columns with cap 0
        assert ctx._lib.bs_preempt_cleared_read(ctx._h, 0, None, None, None, None, None) == INVALID      # NULL n_out
        assert ctx._lib.bs_preempt_cleared_read(None, 0, None, None, None, None, None) == INVALID        # NULL ctx
        before = (_everything(ctx), ctx.preempt_cleared_read())
        twice = np.concatenate([pi[:3], pi[:1]])
        for status, fn in (
                (INVALID, lambda: ctx._preempt_call(CL | soa.PREEMPT_ASSUME, pi, pr_, prot, CAP, soa.STAGE_PREFILTER)),            # ASSUME without APPLY
                (INVALID, lambda: ctx._preempt_call(CL | soa.PREEMPT_NOMINATE, pi, pr_, prot, CAP, soa.STAGE_PREFILTER)),          # NOMINATE without APPLY
                (INVALID, lambda: ctx._preempt_call(CL | 7, pi, pr_, prot, CAP, soa.STAGE_PREFILTER)),                              # NOMINATE with ASSUME
                (INVALID, lambda: ctx._preempt_call(CL | 16, pi, pr_, prot, CAP, soa.STAGE_PREFILTER)),                             # an unknown bit
                (INVALID, lambda: ctx._preempt_call(CL | 1, pi, pr_, prot, CAP, soa.STAGE_PREFILTER, gang=(None, False))),          # gang_need NULL with g > 0
                (INVALID, lambda: ctx.preempt_commit(twice, pr_[:4], prot, victim_cap=CAP, apply=True, clear_lower=True)),          # a pod twice
                (INVALID, lambda: ctx.preempt_commit([sc["pods"].p], [5], prot, victim_cap=CAP, apply=True, clear_lower=True)),     # pod index >= p
                (INVALID, lambda: ctx.preempt_commit_gang(pi, pr_, prot, need, victim_cap=CAP, apply=True, clear_lower=True, stages=3))):
            _refused(status, fn)
            _equal_everything(_everything(ctx), before[0], "after a refusal")
            after = ctx.preempt_cleared_read()
            assert after["n"] == before[1]["n"] and all(np.array_equal(after[f], before[1][f]) for f in cr.CLEARED), "the previous report stays"
        none = ctx.preempt_commit([], [], prot, victim_cap=CAP, clear_lower=True)   # count == 0: a flagged call that clears nothing
        assert none["cleared"]["id"].size == 0 and ctx.preempt_cleared_read(4)["n"] == 0
        ctx.preempt(pi, pr_, prot, victim_cap=CAP)
        _refused(STATE_ERR, ctx.preempt_cleared_read, 0)                          # bs_preempt_run carries no flags


# ---- 6. two cycles on one context ----------------------------------------------------------------------------------------------------------
def test_two_cycles_nominate_clear_bind_and_preempt_again():
    """cycle 1: commit(APPLY | NOMINATE | CLEAR_LOWER) on a table of earlier nominees: rows leave, nominees arrive.  The nominees on even
    nodes bind (out of the table, into the bound table with BS_BOUND_NODES).  Cycle 2: the other preemptors, flagged again, now clearing
    among cycle 1's nominees too.  Every state is held against the model"""
    sc, rows = _scene(472, 2, False, n=24, q=24)                              # (picked on the CPU: both cycles clear rows)
    half = np.arange(24) % 2 == 1                                                 # cycle 2 gets every other preemptor: both halves hold high priorities
    one = dict(sc, pod_index=sc["pod_index"][half], priority=sc["priority"][half])
    two = dict(sc, pod_index=sc["pod_index"][~half], priority=sc["priority"][~half])
    model = _model_table(sc, rows)
    with _ctx(sc, rows) as ctx:
        got = _call(ctx, one, "nominate")
        exp = _expect(one, rows, "nominate")
        _same(got, exp["res"], "cycle 1")
        _same_cleared(got["cleared"], exp["cleared"], "cycle 1")
        ids = cr.table_after(model, exp, one["pod_index"], one["priority"], sc["pods"], True, True)
        assert np.array_equal(got["nominated_id"], ids) and exp["cleared"]["id"].size
        _read_equal(ctx, model.read(), "cycle 1 rows")
        t = model.read()
        binds = np.nonzero((t["node"] % 2 == 0) & (t["id"] >= rows["id"].size))[0]
        assert 0 < binds.size
        ctx.nominated_apply(t["id"][binds])
        model.apply(t["id"][binds], [], [], [], sc["pods"])
        ins = soa.Bound(t["node"][binds], t["priority"][binds], np.full(binds.size, 10 ** 9, np.int64), np.full(binds.size, soa.POD_NOT_GROUPED, np.int32),
                        t["req"][:, binds], t["req_present"][binds])
        first = ctx.bound_apply_ex(None, ins)
        st = _state(ctx)
        keep, b0 = exp["bound_id"], sc["bound"]
        bound2 = soa.Bound(np.concatenate([b0.node[keep], ins.node]), np.concatenate([b0.priority[keep], ins.priority]),
                           np.concatenate([b0.start_ns[keep], ins.start_ns]), np.concatenate([b0.group[keep], ins.group]),
                           np.concatenate([b0.req[:, keep], ins.req], axis=1), np.concatenate([b0.req_present[keep], ins.req_present]))
        sc2 = dict(two, nodes=soa.Nodes(sc["nodes"].allocatable, st["req"], sc["nodes"].allocatable_present, st["pres"], sc["nodes"].flags), bound=bound2,
                   violating=np.concatenate([sc["violating"][keep], np.zeros(binds.size, np.uint8)]))
        left = model.read()
        got2 = _call(ctx, two, "nominate")
        exp2 = _expect(sc2, left, "nominate")
        idmap = np.concatenate([keep, first + np.arange(binds.size, dtype=np.uint32)]).astype(np.uint32)
        for f in ("node", "n_candidates", "n_victims", "top_priority", "priority_sum", "earliest_start", "n_pdb_violations"):
            assert np.array_equal(got2[f], exp2["res"][f]), f"cycle 2: {f}"
        for i in range(len(got2["node"])):
            nv = min(int(got2["n_victims"][i]), CAP)
            assert np.array_equal(got2["victims"][i, :nv], idmap[exp2["res"]["victims"][i, :nv]]), f"cycle 2: victims of {i}"
        _same_cleared(got2["cleared"], exp2["cleared"], "cycle 2")
        ids2 = cr.table_after(model, exp2, two["pod_index"], two["priority"], sc["pods"], True, True)
        assert np.array_equal(got2["nominated_id"], ids2)
        _read_equal(ctx, model.read(), "cycle 2 rows")
        assert np.any(exp2["cleared"]["id"] >= rows["id"].size) and np.any(exp2["cleared"]["id"] < rows["id"].size), "cycle 2 clears old and new rows"
