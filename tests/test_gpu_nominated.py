"""GPU tests of the resident nominated-pod table and of rule N (include/bsched.h; csrc/bs_nominated.hpp: k_nm_mark / k_nm_move / k_nm_gather /
k_nm_chains, and pre_nominees in the victim search of bs_preempt_run, bs_preempt_commit and bs_preempt_commit_gang).

Two kinds of check.  Twin contexts, byte-equal, with no model in between: rows that all qualify equal a twin whose nodes got the rows
through bs_nodes_assume; rows that never qualify equal a twin without a table.  And tests/nominated_ref.py's array statement (held against
the object statement and hand known answers by tests/test_nominated_cpu.py) for mixed priorities.  The shapes are the smallest at which
each mechanism can go wrong: 65 preemptors are two tiles, 96 nodes several chunks, 1023 / 1024 / 1025 rows the compaction's window edge."""
import importlib

import numpy as np
import pytest

import bound_nodes_ref as bn
import extreme_scenes as ex
import nominated_ref as nr
import preempt_commit_paths as paths
import preempt_gang_scenes as gs
import preempt_pdb_ref as pp
from preempt_scenes import groups_for, kat_scene
from test_nominated_cpu import kat_rows, kats

pytestmark = pytest.mark.gpu

bsa = importlib.import_module("batch-scheduler_amd")
soa, capi = bsa.soa, bsa.capi
HOOK = "BS_TEST_PC_CHUNK_NODES"
INVALID, STATE_ERR, CAPACITY = -1, -4, -5
CAP = 8
MODES = ("run", "commit", "gang")
I32_MIN = -(1 << 31)


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _ctx(sc, rows=None, nodes=None):
    ctx = bsa.Context(scalar_lanes=sc["S"], device=0)
    ctx.load_nodes(sc["nodes"] if nodes is None else nodes, sc["fit"])
    ctx.load_groups(groups_for(sc))
    ctx.load_pods(sc["pods"])
    ctx.load_bound(sc["bound"])
    if sc.get("violating") is not None:
        ctx.bound_pdb_set(sc["violating"])
    if rows is not None:
        ctx.nominated_load(rows["node"], rows["priority"], rows["req"], rows["req_present"])
    return ctx


def _scene(seed, S, gang, n=96, q=65, per_node=(2, 6)):
    if gang:
        return gs.gang_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=4, share=0.2)
    sc, bits = pp.pdb_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=4, share=0.2)
    sc["violating"] = bits
    sc["need"] = np.zeros(sc["groups"], np.uint32)
    return sc


def _table(sc, node, prio, req, pres) -> dict:
    t = nr.NomTable(sc["S"])
    t.load(sc["nodes"].n, node, prio, req, pres)
    return t.read()


def _rows_with_priority(rows, prio) -> dict:
    out = {k: v.copy() for k, v in rows.items()}
    out["priority"] = np.asarray(prio, np.int32).reshape(-1).copy() if np.ndim(prio) else np.full(rows["id"].size, prio, np.int32)
    return out


def _call(ctx, mode, sc, apply=False, assume=False, nominate=False, pick=None) -> dict:
    pi, pr_ = (sc["pod_index"], sc["priority"]) if pick is None else (sc["pod_index"][pick], sc["priority"][pick])
    if mode == "run":
        return ctx.preempt(pi, pr_, sc["protected"], victim_cap=CAP)
    if mode == "commit":
        return ctx.preempt_commit(pi, pr_, sc["protected"], victim_cap=CAP, apply=apply, assume=assume, nominate=nominate)
    return ctx.preempt_commit_gang(pi, pr_, sc["protected"], sc["need"], victim_cap=CAP, apply=apply, assume=assume, nominate=nominate)


def _expect(mode, sc, rows, apply=False, assume=False) -> dict:
    prep = pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], sc["violating"])
    a = (prep, sc["fit"], sc["pods"])
    if mode == "run":
        return dict(res=nr.run_nom_np(*a, sc["pod_index"], sc["priority"], sc["protected"], CAP, rows))
    if mode == "commit":
        return nr.commit_nom_np(*a, sc["bound"], sc["pod_index"], sc["priority"], sc["protected"], CAP, rows, apply, assume)
    return nr.gang_nom_np(*a, sc["bound"], sc["pod_index"], sc["priority"], sc["protected"], sc["need"], CAP, rows, apply, assume)


def _same(got, exp, where, fields=pp.FIELDS):
    for f in fields:
        if f in exp and not np.array_equal(got[f], exp[f]):
            bad = np.nonzero(np.any((np.asarray(got[f]) != np.asarray(exp[f])).reshape(len(got[f]), -1), axis=1))[0]
            i = int(bad[0])
            pytest.fail(f"{where}: {f} differs at {i} of {len(bad)} bad: got {got[f][i]} expected {exp[f][i]}")


def _state(ctx) -> dict:
    req, pres = ctx.read_node_requests()
    ids, nodes = ctx.read_bound()
    return dict(req=req, pres=pres, bound_id=ids, bound_node=nodes)


def _check_against_ref(ctx, mode, sc, rows, apply, assume, where):
    got = _call(ctx, mode, sc, apply, assume)
    exp = _expect(mode, sc, rows, apply, assume)
    _same(got, exp["res"], where)
    if mode != "run":
        _same(_state(ctx), exp, where + " state", gs.STATE)
    if mode == "gang":
        _same(got, exp, where, ("slot_voided", "group_placed"))
    return got


def _eff(req, pres):
    """effective requests: a scalar lane without its present bit counts 0"""
    out = np.array(req, np.int64, copy=True)
    for l in range(4, out.shape[0]):
        out[l] = np.where((np.asarray(pres) >> np.uint32(l - 4)) & 1, out[l], 0)
    return out


def _assumed_nodes(sc, rows):
    """the scene's nodes with every row added to its node's requests (AddPod), and the (index, lanes, present) records that do it"""
    L, n = 4 + sc["S"], sc["nodes"].n
    with np.errstate(over="ignore"):
        total = _eff(sc["nodes"].requested, sc["nodes"].requested_present) + nr.NomSums(rows, L, n)(I32_MIN)
    pres = np.array(sc["nodes"].requested_present, np.uint32, copy=True)
    np.bitwise_or.at(pres, rows["node"].astype(np.int64), rows["req_present"])
    recs = [(int(k), total[:, k].tolist(), int(pres[k])) for k in np.unique(rows["node"])]
    return total, pres, recs


def _read_equal(ctx, exp: dict, where):
    got = ctx.nominated_read()
    assert ctx.nominated_count() == exp["id"].size, where
    for f in exp:
        assert np.array_equal(got[f], exp[f]), f"{where}: {f}: {got[f].tolist()[:24]} vs {exp[f].tolist()[:24]}"


def _refused(status, fn, *a, **kw):
    with pytest.raises(capi.BsError) as e:
        fn(*a, **kw)
    assert e.value.status == status, str(e.value)


# ---- 1. the hand known answers ---------------------------------------------------------------------------------------------------------
def test_hand_known_answers_on_device():
    for k in kats():
        s = kat_scene(k)
        s["violating"], s["need"] = None, np.array(k.get("need", [0] * s["groups"]), np.uint32)
        rows = kat_rows(k).read()

        def check(res, expect, where):
            for i, e in enumerate(expect):
                nv = int(res["n_victims"][i])
                assert (int(res["node"][i]), int(res["n_candidates"][i]), res["victims"][i, :nv].tolist()) == (e["node"], e["n_candidates"], e["victims"]), \
                    f"{k['name']} {where} preemptor {i}"

        if k["call"] == "run":
            with _ctx(s, rows) as ctx:
                check(_call(ctx, "run", s), k["expect"], "run")
        elif k["call"] == "gang":
            with _ctx(s, rows) as ctx:
                got = _call(ctx, "gang", s, apply=True, nominate=True)
                check(got, k["expect"], "gang")
                assert got["slot_voided"].tolist() == k["expect_voided"] and np.all(got["nominated_id"] == capi.NOM_NONE)
                assert ctx.nominated_count() == k["expect_rows"]
        else:
            second = dict(s, pod_index=np.array(k["second"]["pod_index"], np.uint32), priority=np.array(k["second"]["priority"], np.int32))
            for flag in ("nominate", "assume"):
                with _ctx(s, rows) as ctx:
                    first = _call(ctx, "commit", s, apply=True, assume=flag == "assume", nominate=flag == "nominate")
                    check(first, k["expect_first"], flag + " first")
                    if flag == "nominate":
                        assert first["nominated_id"].tolist() == [0] and ctx.nominated_count() == 1
                    check(_call(ctx, "run", second), k["expect_" + flag], flag + " second")


# ---- 2. equivalence by twin contexts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_rows_that_all_qualify_equal_a_twin_with_assumed_nodes(mode):
    """(a) every row's priority >= every preemptor's: the twin has no table, its nodes got the rows through bs_nodes_assume.  After APPLY
    the node requests of the two differ by exactly the row sums, and bs_bound_dump is equal"""
    sc = _scene(11, 2, mode == "gang")
    rows = _rows_with_priority(nr.nom_rows_for(sc, 11, density=0.4), int(sc["priority"].max()))
    total, pres, recs = _assumed_nodes(sc, rows)
    apply = mode != "run"
    with _ctx(sc, rows) as ctx, _ctx(sc) as twin:
        twin.assume_nodes(recs)
        got, want = _call(ctx, mode, sc, apply=apply), _call(twin, mode, sc, apply=apply)
        _same(got, want, f"(a) {mode}")
        if mode == "gang":
            _same(got, want, "(a) gang", ("slot_voided", "group_placed"))
        assert np.any(got["n_victims"] != _expect(mode, sc, None, apply)["res"]["n_victims"]), "the rows change nothing: the twin proves little"
        a, b = _state(ctx), _state(twin)
        with np.errstate(over="ignore"):
            assert np.array_equal(_eff(a["req"], a["pres"]) + nr.NomSums(rows, 4 + sc["S"], sc["nodes"].n)(I32_MIN), _eff(b["req"], b["pres"]))
        assert np.array_equal(a["bound_id"], b["bound_id"]) and np.array_equal(a["bound_node"], b["bound_node"])
        da, db = ctx.bound_dump(), twin.bound_dump()
        for f in da:
            assert np.array_equal(da[f], db[f]), f"(a) {mode}: bs_bound_dump {f}"


@pytest.mark.parametrize("mode", MODES)
def test_rows_that_never_qualify_equal_a_twin_without_a_table(mode):
    """(b) every row's priority is below every preemptor's: outputs and resident state are byte-equal to a context with no table"""
    sc = _scene(12, 2, mode == "gang")
    rows = _rows_with_priority(nr.nom_rows_for(sc, 12, density=0.9), int(sc["priority"].min()) - 1)
    apply = mode != "run"
    with _ctx(sc, rows) as ctx, _ctx(sc) as twin:
        got, want = _call(ctx, mode, sc, apply=apply, assume=apply), _call(twin, mode, sc, apply=apply, assume=apply)
        _same(got, want, f"(b) {mode}")
        _same(_state(ctx), _state(twin), f"(b) {mode} state", gs.STATE)
        _read_equal(ctx, rows, "(b): the table is not touched")


def test_mixed_priorities_group_by_group_equal_their_own_twins():
    """(c) bs_preempt_run with mixed priorities: the preemptors grouped by which rows qualify; each group equals its own twin of form (a)"""
    sc = _scene(13, 0, False)
    rows = nr.nom_rows_for(sc, 13, density=0.5)
    with _ctx(sc, rows) as ctx:
        got = _call(ctx, "run", sc)
    differs = 0
    for P in np.unique(sc["priority"]):
        pick = np.nonzero(sc["priority"] == P)[0]
        sel = rows["priority"] >= P
        part = {k: (v[:, sel] if k == "req" else v[sel]) for k, v in rows.items()}
        with _ctx(sc) as twin:
            if sel.any():
                twin.assume_nodes(_assumed_nodes(sc, part)[2])
            want = _call(twin, "run", sc, pick=pick)
        _same({f: got[f][pick] for f in pp.FIELDS}, want, f"(c) priority {P}")
        differs += int(sel.any() and not sel.all())
    assert differs, "no group sees a proper subset of the rows"


# ---- 3. against nominated_ref ---------------------------------------------------------------------------------------------------------------
def _ref_scene(seed, S, gang):
    """65 preemptors (two tiles) on 96 nodes with PDB bits; rows on a third of the nodes with priorities around the preemptors', plus 4 rows
    on ONE node straddling a preemptor's priority with two ties at it, rows on a flagged node and rows on a node whose fit bits are clear"""
    sc = _scene(seed, S, gang)
    fitb = sc["fit"].to_bool()
    busy = int(np.argmax(np.bincount(sc["bound"].node.astype(np.int64), minlength=96)))
    flagged, unfit = (busy + 7) % 96, (busy + 13) % 96
    sc["nodes"].flags[flagged] = 1
    fitb[:, unfit] = False
    fitb[:, busy] = True
    sc["nodes"].flags[busy] = 0
    sc["fit"] = soa.FitMasks.from_bool(fitb)
    base = nr.nom_rows_for(sc, seed, density=0.33)
    P0 = int(np.median(sc["priority"]))
    rng = np.random.default_rng(seed)
    src = rng.integers(0, sc["pods"].p, size=8)
    node = np.concatenate([base["node"], [busy] * 4, [flagged] * 2, [unfit] * 2]).astype(np.uint32)
    prio = np.concatenate([base["priority"], [P0 + 1, P0, P0, P0 - 1], [P0, P0 + 1], [P0, P0 + 1]]).astype(np.int32)
    req = np.concatenate([base["req"], sc["pods"].req[: 4 + S, src]], axis=1)
    pres = np.concatenate([base["req_present"], sc["pods"].req_present[src]]).astype(np.uint32)
    return sc, _table(sc, node, prio, req, pres)


@pytest.mark.parametrize("S", [0, 2, 12])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_priorities_against_the_reference(mode, S):
    sc, rows = _ref_scene(21 + S, S, mode == "gang")
    bare = _expect(mode, sc, None)["res"]
    for apply, assume in ((False, False), (True, True)) if mode != "run" else ((False, False),):
        with _ctx(sc, rows) as ctx:
            got = _check_against_ref(ctx, mode, sc, rows, apply, assume, f"{mode} S={S} apply={apply}")
            _read_equal(ctx, rows, "the table is static within a call")
    assert nr.changed(got, bare), "the rows change no answer of this scene"


@pytest.mark.parametrize("S,seed,cn", [(0, 39, 5), (12, 41, 8)])
def test_resolve_fallback_and_rescan_paths_with_rows_in_dirty_chunks(S, seed, cn, monkeypatch):
    """chunks of several nodes (the hook), so that the resolve pass takes later record entries (cn nodes a chunk) and rescans chunks (all 96
    nodes one chunk), as tests/test_gpu_preempt_commit_chunks.py establishes the two paths; a dirty node sits in the same chunk as a node
    that holds a row.  The seeds were picked on the CPU for that.
    Part 1: rows that all qualify — the path classifier runs on the equivalent scene (nodes with the rows assumed), where it is exact.
    Part 2: the same scene and hooks with mixed row priorities, against the reference."""
    sc, rows = _ref_scene(seed, S, False)
    allq = _rows_with_priority(rows, int(sc["priority"].max()))
    total, pres, _ = _assumed_nodes(sc, allq)
    eq = dict(sc, nodes=soa.Nodes(sc["nodes"].allocatable, total, sc["nodes"].allocatable_present, pres, sc["nodes"].flags))
    plan = _expect("commit", eq, None)
    few, one = paths.classify(eq, plan["res"], cn, bits=sc["violating"]), paths.classify(eq, plan["res"], 96, bits=sc["violating"])
    assert few["later"] > 0 and one["nchunks"] == 1 and one["rescans"] > 0, paths.summary(few) + " | " + paths.summary(one)
    chosen = plan["res"]["node"][plan["res"]["node"] >= 0]
    holders = np.unique(allq["node"])
    assert any(h != k and h // cn == k // cn for k in chosen for h in holders), "no dirty node shares a chunk with a node that holds a row"
    for hook in (cn, 96):
        monkeypatch.setenv(HOOK, str(hook))
        for r in (allq, rows):
            for mode in ("commit", "gang"):
                with _ctx(sc, r) as ctx:
                    _check_against_ref(ctx, mode, sc, r, True, False, f"{HOOK}={hook} S={S} {mode}")
        with _ctx(sc, rows) as ctx:
            _check_against_ref(ctx, "run", sc, rows, False, False, f"{HOOK}={hook} S={S} run")


def test_row_sums_that_wrap_int64():
    """one scene whose row sums wrap: two rows of I64_MAX and one of SAFE on a node pass through zero and back; the victim search sees the
    wrapped sum the model sees (library rule N1), and APPLY stores none of it"""
    sc = _scene(41, 1, False, n=24, q=20)
    k = int(np.argmax(np.bincount(sc["bound"].node.astype(np.int64), minlength=24)))
    L = 5
    req = np.zeros((L, 4), np.int64)
    req[0] = [ex.I64_MAX, ex.I64_MAX, 2, ex.SAFE]
    req[1] = [ex.I64_MIN + 1, ex.I64_MAX, 0, 0]
    req[4] = [ex.I64_MAX, ex.SAFE, ex.SAFE, 0]
    rows = _table(sc, [k, k, k, (k + 1) % 24], [int(sc["priority"].max())] * 4, req, [1, 1, 1, 0])
    for mode in ("run", "commit"):
        with _ctx(sc, rows) as ctx:
            _check_against_ref(ctx, mode, sc, rows, mode == "commit", False, f"wrap {mode}")


# ---- 4. table mechanics ------------------------------------------------------------------------------------------------------------------
def _small(S=2):
    return _scene(51, S, False, n=24, q=12)


def test_apply_equals_load_of_the_models_arrays():
    sc = _small()
    rng = np.random.default_rng(5)
    model = nr.NomTable(sc["S"])
    first = nr.nom_rows_for(sc, 5, density=0.5)
    model.load(24, first["node"], first["priority"], first["req"], first["req_present"])
    with _ctx(sc, first) as ctx, _ctx(sc) as fresh:
        for step in range(4):
            remove = rng.permutation(model.id)[: int(rng.integers(0, model.id.size))]
            ni = int(rng.integers(0, 9))
            pod, node, prio = rng.integers(0, sc["pods"].p, size=ni), rng.integers(0, 24, size=ni), rng.integers(-9, 6000, size=ni)
            assert ctx.nominated_apply(remove, pod, node, prio) == model.apply(remove, pod, node, prio, sc["pods"])
            exp = model.read()
            _read_equal(ctx, exp, f"step {step}")
            assert ctx.nominated_ids() == model.ids
            fresh.nominated_load(exp["node"], exp["priority"], exp["req"], exp["req_present"])
            got = fresh.nominated_read()
            assert all(np.array_equal(got[f], exp[f]) for f in ("node", "priority", "req", "req_present")), "load stores what apply stored"
        assert ctx.nominated_apply() == model.ids and ctx.nominated_count() == model.id.size     # both counts 0: BS_OK, nothing changes


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_removals_across_the_compaction_window_edge(m):
    """1023, 1024 and 1025 rows through a removal (k_nm_move walks windows of 1024 with a running base); the first row, the last row, rows
    on both sides of the edge, and then every row"""
    sc = _small(S=1)
    rng = np.random.default_rng(m)
    src = rng.integers(0, sc["pods"].p, size=m)
    rows = _table(sc, rng.integers(0, 24, size=m), rng.integers(0, 6000, size=m), sc["pods"].req[:5, src], sc["pods"].req_present[src])
    model = nr.NomTable(1)
    model.load(24, rows["node"], rows["priority"], rows["req"], rows["req_present"])
    with _ctx(sc, rows) as ctx:
        for remove in ([0], [m - 1], [x for x in (1022, 1023, 1024) if 0 < x < m - 1], list(rng.permutation(np.arange(1, m - 1))[:300])):
            remove = [r for r in remove if r in set(model.id.tolist())]
            ctx.nominated_apply(remove)
            model.apply(remove, [], [], [], sc["pods"])
            _read_equal(ctx, model.read(), f"m={m} remove {remove[:4]}")
        ctx.nominated_apply(model.id)
        assert ctx.nominated_count() == 0 and ctx.nominated_ids() == m
        ctx.nominated_apply([], [3], [2], [7])
        assert ctx.nominated_read()["id"].tolist() == [m], "ids are not reused"


def test_an_insert_that_outgrows_the_headroom():
    sc = _small()
    first = nr.nom_rows_for(sc, 6, density=0.3)
    model = nr.NomTable(sc["S"])
    model.load(24, first["node"], first["priority"], first["req"], first["req_present"])
    rng = np.random.default_rng(6)
    with _ctx(sc, first) as ctx:
        for ni in (300, 900):                                # a small load leaves room for 256 rows: both inserts outgrow their allocation
            pod, node, prio = rng.integers(0, sc["pods"].p, size=ni), rng.integers(0, 24, size=ni), rng.integers(0, 6000, size=ni)
            assert ctx.nominated_apply([], pod, node, prio) == model.apply([], pod, node, prio, sc["pods"])
            _read_equal(ctx, model.read(), f"insert {ni}")
        rows = model.read()
        _check_against_ref(ctx, "run", sc, rows, False, False, "after growing")


@pytest.mark.parametrize("mode", ["commit", "gang"])
def test_nominate_appends_the_slots_that_hold_a_node(mode):
    sc = _scene(61, 2, mode == "gang", n=24, q=20)
    first = nr.nom_rows_for(sc, 61, density=0.3)
    model = nr.NomTable(2)
    model.load(24, first["node"], first["priority"], first["req"], first["req_present"])
    with _ctx(sc, first) as ctx:
        got = _call(ctx, mode, sc, apply=True, nominate=True)
        exp = _expect(mode, sc, first, True, False)
        _same(got, exp["res"], f"nominate {mode}")
        _same(_state(ctx), exp, "APPLY | NOMINATE leaves the node requests APPLY leaves", gs.STATE)
        ids = nr.nominate_rows(model, exp["res"], sc["pod_index"], sc["priority"], sc["pods"])
        assert np.array_equal(got["nominated_id"], ids) and np.any(ids == nr.NONE) and np.any(ids != nr.NONE)
        if mode == "gang":
            assert np.any(got["slot_voided"] != 0) and np.all(ids[got["slot_voided"] != 0] == nr.NONE), "a voided slot nominates nobody"
        _read_equal(ctx, model.read(), "the appended rows")
        assert np.array_equal(ctx.preempt_nominated_read(20), ids)
        _refused(INVALID, ctx.preempt_nominated_read, 19)
        _call(ctx, "run", sc)
        _refused(STATE_ERR, ctx.preempt_nominated_read, 20)      # the last preemption call did not carry the flag


def test_chains_rebuilt_after_removals_answer_like_a_fresh_load_of_the_survivors():
    sc, rows = _ref_scene(71, 2, False)
    model = nr.NomTable(2)
    model.load(96, rows["node"], rows["priority"], rows["req"], rows["req_present"])
    remove = model.id[::3]
    model.apply(remove, [], [], [], sc["pods"])
    left = model.read()
    with _ctx(sc, rows) as ctx, _ctx(sc, left) as fresh:
        ctx.nominated_apply(remove)
        for mode in ("run", "commit"):
            _same(_call(ctx, mode, sc), _call(fresh, mode, sc), f"survivors {mode}")
        _check_against_ref(ctx, "commit", sc, left, False, False, "survivors against the reference")


# ---- 5. two full cycles on one context ------------------------------------------------------------------------------------------------------
def test_two_cycles_nominate_bind_and_preempt_again():
    """commit(APPLY | NOMINATE); the nominees that bind leave the table (bs_nominated_apply) and enter the bound table WITH BS_BOUND_NODES
    (now they are in the node requests); a second commit.  Every state is held against the model"""
    sc = _scene(81, 2, False, n=24, q=24)
    half = np.arange(24) < 12
    one, two = dict(sc, pod_index=sc["pod_index"][half], priority=sc["priority"][half]), dict(sc, pod_index=sc["pod_index"][~half], priority=sc["priority"][~half])
    model = nr.NomTable(2)
    model.load(24, [], [], np.zeros((6, 0)), [])
    with _ctx(sc, model.read()) as ctx:
        got = _call(ctx, "commit", one, apply=True, nominate=True)
        exp = _expect("commit", one, model.read(), True, False)
        _same(got, exp["res"], "cycle 1")
        ids = nr.nominate_rows(model, exp["res"], one["pod_index"], one["priority"], sc["pods"])
        assert np.array_equal(got["nominated_id"], ids)
        _read_equal(ctx, model.read(), "cycle 1 rows")
        # the nominees on even nodes bind on their nodes
        rows = model.read()
        binds = np.nonzero(rows["node"] % 2 == 0)[0]
        assert 0 < binds.size < rows["id"].size
        ctx.nominated_apply(rows["id"][binds])
        model.apply(rows["id"][binds], [], [], [], sc["pods"])
        ins = soa.Bound(rows["node"][binds], rows["priority"][binds], np.full(binds.size, 10 ** 9, np.int64), np.full(binds.size, soa.POD_NOT_GROUPED, np.int32),
                        rows["req"][:, binds], rows["req_present"][binds])
        first = ctx.bound_apply_ex(None, ins)
        st = _state(ctx)
        # the model's state after cycle 1: the survivors of the bound table in table order plus the inserts, the nodes with the binders added
        keep = exp["bound_id"]
        b0 = sc["bound"]
        bound2 = soa.Bound(np.concatenate([b0.node[keep], ins.node]), np.concatenate([b0.priority[keep], ins.priority]),
                           np.concatenate([b0.start_ns[keep], ins.start_ns]), np.concatenate([b0.group[keep], ins.group]),
                           np.concatenate([b0.req[:, keep], ins.req], axis=1), np.concatenate([b0.req_present[keep], ins.req_present]))
        with np.errstate(over="ignore"):
            req2 = _eff(exp["req"], exp["pres"]) + nr.NomSums(dict(rows, node=rows["node"][binds], priority=rows["priority"][binds], req=rows["req"][:, binds],
                                                                   id=rows["id"][binds], req_present=rows["req_present"][binds]), 6, 24)(I32_MIN)
        assert np.array_equal(_eff(st["req"], st["pres"]), req2), "BS_BOUND_NODES adds the binders to their nodes"
        # cycle 2 on the device against the model on a scene rebuilt from the model's state (ids renumbered: keep, then the inserts)
        sc2 = dict(two, nodes=soa.Nodes(sc["nodes"].allocatable, st["req"], sc["nodes"].allocatable_present, st["pres"], sc["nodes"].flags), bound=bound2,
                   violating=np.concatenate([sc["violating"][keep], np.zeros(binds.size, np.uint8)]))
        got2 = _call(ctx, "commit", two, apply=True, nominate=True)
        exp2 = _expect("commit", sc2, model.read(), True, False)
        idmap = np.concatenate([keep, first + np.arange(binds.size, dtype=np.uint32)]).astype(np.uint32)
        for f in ("node", "n_candidates", "n_victims", "top_priority", "priority_sum", "earliest_start", "n_pdb_violations"):
            assert np.array_equal(got2[f], exp2["res"][f]), f"cycle 2: {f}"
        for i in range(len(got2["node"])):
            nv = min(int(got2["n_victims"][i]), CAP)
            assert np.array_equal(got2["victims"][i, :nv], idmap[exp2["res"]["victims"][i, :nv]]), f"cycle 2: victims of {i}"
        ids2 = nr.nominate_rows(model, exp2["res"], two["pod_index"], two["priority"], sc["pods"])
        assert np.array_equal(got2["nominated_id"], ids2)
        _read_equal(ctx, model.read(), "cycle 2 rows")
        st2 = _state(ctx)
        assert np.array_equal(_eff(st2["req"], st2["pres"]), _eff(exp2["req"], exp2["pres"])) and np.array_equal(st2["bound_id"], idmap[exp2["bound_id"]])


# ---- 6. refusals and the stale node count ----------------------------------------------------------------------------------------------------
def test_every_refused_call_changes_nothing():
    sc = _small()
    rows = nr.nom_rows_for(sc, 7, density=0.5)
    with _ctx(sc) as ctx:
        _refused(STATE_ERR, ctx.nominated_count)
        _refused(STATE_ERR, ctx.nominated_apply, [], [0], [0], [1])
        _refused(STATE_ERR, _call, ctx, "commit", sc, True, False, True)                      # NOMINATE needs a table
        ctx.nominated_load(rows["node"], rows["priority"], rows["req"], rows["req_present"])
        ctx.nominated_apply([1, 2])
        model = nr.NomTable(sc["S"])
        model.load(24, rows["node"], rows["priority"], rows["req"], rows["req_present"])
        model.apply([1, 2], [], [], [], sc["pods"])
        before = (model.read(), _state(ctx), ctx.bound_dump())
        m, p = rows["id"].size, sc["pods"].p
        for status, fn, a, kw in (
                (INVALID, ctx.nominated_apply, ([1],), {}),                                    # dead
                (INVALID, ctx.nominated_apply, ([m],), {}),                                    # unknown
                (INVALID, ctx.nominated_apply, ([0, 3, 0],), {}),                              # repeated
                (INVALID, ctx.nominated_apply, ([], [p], [0], [1]), {}),                       # pod_index >= p
                (INVALID, ctx.nominated_apply, ([0], [0], [24], [1]), {}),                     # node >= n, with a valid removal beside it
                (INVALID, ctx.nominated_apply, (), dict(n_remove=2)),                          # NULL with a count
                (INVALID, ctx.nominated_apply, (), dict(n_insert=1)),
                (CAPACITY, ctx.nominated_load, ([0], [1], None, None), dict(m=capi.NOM_MAX + 1)),
                (INVALID, ctx.nominated_load, ([24], [1]), {}),
                (INVALID, _call, (ctx, "commit", sc, False, False, True), {}),                 # NOMINATE without APPLY
                (INVALID, _call, (ctx, "commit", sc, True, True, True), {}),                   # NOMINATE with ASSUME
                (INVALID, _call, (ctx, "gang", sc, True, True, True), {})):
            _refused(status, fn, *a, **kw)
            _read_equal(ctx, before[0], "after a refusal")
            st, dump = _state(ctx), ctx.bound_dump()
            assert all(np.array_equal(st[f], before[1][f]) for f in st) and all(np.array_equal(dump[f], before[2][f]) for f in dump)
        sharded = bsa.Context(scalar_lanes=sc["S"], device=0)
        with sharded:
            sharded.load_nodes(sc["nodes"], sc["fit"])
            sharded.set_shard(0, 2)
            _refused(STATE_ERR, sharded.nominated_load)


def test_a_stale_node_count_is_refused_while_the_table_holds_rows():
    sc = _small()
    rows = nr.nom_rows_for(sc, 8, density=0.5)
    nl = bn.NodeList(sc["nodes"], sc["fit"])
    d = nl.append(3)
    grown = dict(sc, nodes=nl.nodes(), fit=nl.fit())
    with _ctx(sc, rows) as ctx, _ctx(sc, _table(sc, [], [], np.zeros((4 + sc["S"], 0)), [])) as empty, _ctx(grown) as twin:
        for c in (ctx, empty):
            c.apply_node_deltas([d])
            c.bound_nodes_apply([bn.APPEND], [0])
        for mode in MODES:
            _refused(STATE_ERR, _call, ctx, mode, sc)
            _same(_call(empty, mode, sc), _call(twin, mode, sc), f"an empty stale table: {mode} behaves as without one")
        _refused(STATE_ERR, ctx.nominated_read)
        _refused(STATE_ERR, ctx.nominated_apply, [0])
        _refused(STATE_ERR, _call, empty, "commit", sc, True, False, True)                    # NOMINATE needs a table for THIS node count
        assert ctx.nominated_count() == rows["id"].size and ctx.nominated_ids() == rows["id"].size
        # the documented way through: read before the surgery (here: the caller's copy), remap on the host, load
        ctx.nominated_load(rows["node"], rows["priority"], rows["req"], rows["req_present"])
        _same(_call(ctx, "run", grown), _expect("run", grown, rows)["res"], "after the reload")
