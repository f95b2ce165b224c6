"""GPU tests of the sequential pass against the hand-derived answers of tests/golden/seq_hand_kats.json, on every form the body of
bs_seq_pass.inc is compiled into: bs_seq_run and bs_seq_run_flat, bs_seq_run_nominated (empty table, no own ids) and its flat twin,
bs_seq_run_scored with weights (0, 0, 0), bs_seq_run_scored_nominated with both.  The whole record, bit-exact, against the JSON — not against
the oracle: every pod's code, first_k and stale leader, the node of every released pod, the gangs in release order, the node requests and
the group state the pass leaves (tests/test_seq_hand_cpu.py holds the same answers against three CPU models and shows which device path
each scene reaches).  The two Filter scenes run on the forms that take BS_STAGE_FILTER (the nominated forms refuse it)."""
import ctypes as C

import numpy as np
import pytest

import seq_hand_scenes as shs
from test_gpu_parity import load_ctx
from test_gpu_seq import assert_groups_equal, check_pass

pytestmark = pytest.mark.gpu

SCENES = [k for k in shs.load() if not k.get("cpu_only")]
FORMS = ("run", "run_flat", "nominated", "nominated_flat", "scored", "scored_nominated")
FILTER_FORMS = ("run", "run_flat", "scored")
CASES = [(k, f) for k in SCENES for f in (FILTER_FORMS if k.get("stages") == "filter_deny" else FORMS)]


class Form:
    """a context seen through one form of the pass: check_pass calls seq_run and reads the state back"""

    def __init__(self, bsa, ctx, form, cap):
        self.bsa, self.ctx, self.form, self.cap = bsa, ctx, form, cap
        self.read_node_requests, self.read_groups = ctx.read_node_requests, ctx.read_groups
        if "nominated" in form:
            ctx.nominated_load()                                # an empty table

    def seq_run(self, stages):
        ctx, form, cap = self.ctx, self.form, self.cap
        prio = np.zeros(ctx.pods_count(), np.int32)
        if form == "run":
            return ctx.seq_run(stages, cap=cap)
        if form == "run_flat":
            return self._run_flat(stages)
        if form in ("nominated", "nominated_flat"):
            return ctx.seq_run_nominated(prio, None, stages=stages, cap=cap, flat=form.endswith("flat"))
        if form == "scored":
            return ctx.seq_run_scored((0, 0, 0), stages=stages, cap=cap)
        return ctx.seq_run_scored_nominated((0, 0, 0), prio, None, stages=stages, cap=cap)

    def _run_flat(self, stages):
        ctx = self.ctx
        p, cap = ctx.pods_count(), max(ctx.g if self.cap is None else self.cap, 1)
        pf, fk, ld, node, lp = np.zeros(p, np.uint8), np.zeros(p, np.uint32), np.zeros(p, np.int32), np.full(p, -1, np.int32), np.zeros(p, np.uint8)
        rg, rp, t0, t1, sc = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(8, np.int64)
        u8, i32, u32, i64 = ((lambda a, t=t: a.ctypes.data_as(C.POINTER(t))) for t in (C.c_uint8, C.c_int32, C.c_uint32, C.c_int64))
        ctx._chk(ctx._lib.bs_seq_run_flat(ctx._h, stages, u8(pf), u32(fk), i32(ld), i32(node), cap, u32(rg), u32(rp), i64(t0), i64(t1), i64(sc), u8(lp)),
                 "bs_seq_run_flat")
        k = min(int(sc[0]), cap)
        return dict(pf_code=pf, pf_first_k=fk, pf_leader=ld, pod_node=node, last_permitted=lp, released_group=rg[:k], released_pods=rp[:k], first_ns=t0[:k],
                    ready_ns=t1[:k], n_released=int(sc[0]), total_ns=int(sc[1]))


def run_scene(bsa, soa, k, form):
    nodes, fit, groups, pods = shs.to_soa(k, 0)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        f = Form(bsa, ctx, form, k.get("cap"))
        for j in range(len(k["passes"])):
            if j:                                               # the queue is replaced; nodes, groups and the leader are what the last pass left
                ctx.apply_pods(remove=np.arange(ctx.pods_count(), dtype=np.uint32), insert=shs.to_soa(k, j)[3])
            s = shs.expected(k, j, device=True)
            r = check_pass(f, s, soa, f"{k['name']} pass {j} on {form}")
            assert r["n_released"] == s["n_released"] and len(r["released_group"]) == len(s["released_group"])
            released = np.nonzero(r["pod_node"] >= 0)[0]
            assert np.array_equal(r["pod_node"][released], s["assumed"][released]), "a released pod is released on the node it was assumed on"
            if "last_permitted" in r and not s["stages"] & soa.BATCH_FILTER_DENY:
                assert not r["last_permitted"].any()


@pytest.mark.parametrize("k,form", CASES, ids=[f"{k['name']}-{f}" for k, f in CASES])
def test_hand_answers_on_every_form(k, form, bsa, soa):
    run_scene(bsa, soa, k, form)


@pytest.mark.parametrize("slots", ["0", "1"], ids=["round-scan", "one-slot"])
@pytest.mark.parametrize("k", [k for k in SCENES if k["kind"] == "A"], ids=lambda k: k["name"])
def test_semantic_scenes_under_the_scan_variants(k, slots, bsa, soa, monkeypatch):
    """the A scenes without table summaries and with one summary slot, as test_gpu_seq.test_seq_pass_scan_variants runs its scenes"""
    monkeypatch.setenv("BS_SEQ_CACHE_SLOTS", slots)
    run_scene(bsa, soa, k, "run")


@pytest.mark.parametrize("form", FORMS)
def test_tile_scene_without_cursors(form, bsa, soa, monkeypatch):
    """tile_63_64 once more with the first-fit cursors off (the parametrised run above has them on)"""
    monkeypatch.setenv("BS_SEQ_NO_CURSOR", "1")
    (k,) = [k for k in SCENES if "BS_SEQ_NO_CURSOR" in k.get("variants", [])]
    run_scene(bsa, soa, k, form)


def test_short_cap_leaves_the_rest_complete(bsa, soa):
    """cap_1: n_released counts the three gangs, the arrays name the first; pod_node and the group state are complete (check_pass) — and the
    same call with room for all three names all three"""
    (k,) = [k for k in SCENES if k.get("cap") == 1]
    s = shs.expected(k, 0, device=True)
    assert s["n_released"] == 3 and s["released_group"].tolist() == [0] and s["released_pods"].tolist() == [1]
    nodes, fit, groups, pods = shs.to_soa(k, 0)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        r = ctx.seq_run(soa.STAGE_PREFILTER)
        full = shs.expected(k, 0)
        assert r["released_group"].tolist() == full["released_group"].tolist() and r["released_pods"].tolist() == full["released_pods"].tolist()
        assert_groups_equal(ctx.read_groups(), full["groups"], soa, "cap_1 with room")
