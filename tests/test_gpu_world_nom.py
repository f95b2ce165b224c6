"""The nominated-pod table, BS_PREEMPT_NOMINATE / BS_PREEMPT_CLEAR_LOWER, bs_seq_run_nominated and bs_seq_run_scored across MANY calls on one
context, against the composite model of tests/world_ref.py: the second plan family (plan_nom, whose counts tests/test_world_nom_cpu.py
asserts on the model alone) replayed through the Runner of tests/test_gpu_world.py — every call's results field for field, every cheap read
after every call, a context loaded afresh every 8th step —, and the header's cycle with nomination scripted twice: once with the table's own
device paths and once the host way, and once with the scored pass in place of first fit."""
import numpy as np
import pytest

import nominated_nodes_ref as nnr
import seq_soa_ref as ssoa
import world_ref as wf
from test_gpu_world import NOM_COLUMNS, Runner

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(wf.NOM_SEEDS))
def test_many_cycles_with_the_nominated_table(seed, bsa, soa, orc):
    sc, steps = wf.plan_nom(seed, orc)
    with Runner(bsa, soa, orc, sc, f"nom seed {seed}") as r:
        for i, (kind, args, refused) in enumerate(steps):
            r.do(kind, args, refused, flat=bool(i % 2))
            if i % 8 == 7 or i == len(steps) - 1:
                r.against_fresh()


# ---- the header's cycle with nomination, scripted ------------------------------------------------------------------------------------------
def _preemptors(w, dr, cap=12):
    """the pods the last pass left without a node, each gang one run at its group's priority; a gang needs what it sends at most"""
    idx = w.unplaced[:cap]
    grp, prio = w.pods.group[idx], dr._prio(idx)
    o = wf.capi.gang_order(grp, prio)
    idx, grp, prio = idx[o], grp[o], prio[o]
    waiting = np.bincount(w.wt.group, minlength=w.g)[: w.g]
    need = np.minimum(wf.capi.gang_need(w.groups, waiting), np.bincount(grp, minlength=w.g)[: w.g]).astype(np.uint32)
    return dict(pod_index=idx.astype(np.uint32), priority=prio, protected=np.zeros(w.g, np.uint8), need=need, apply=True, assume=False)


def _nominating_cycle(bsa, soa, orc, how):
    """three cycles on scene(9): bs_pods_apply (the nominees stay in the queue) -> the pass (rule S from cycle 2 on, with the own ids of the
    earlier commits) -> bs_bound_bind -> bs_wait_park -> bs_preempt_commit_gang(APPLY | NOMINATE | CLEAR_LOWER).  Between cycles 2 and 3 a node
    that holds rows leaves.  how = "device": BS_PREEMPT_NOMINATE appends the nominees and bs_nominated_nodes_apply follows the surgery.
    how = "host": the commit carries APPLY | CLEAR_LOWER only and bs_nominated_apply appends the nominees; after the surgery the table is read,
    remapped on the host and loaded again (its ids restart: the caller's map goes through the id map)."""
    sc = wf.scene(9)
    rng = np.random.default_rng(199)
    seen = dict(consumed=0, cleared=0, nominated=0, dropped=0, blocked=0, victims=0)
    with Runner(bsa, soa, orc, sc, f"the cycle with nomination ({how})") as r:
        w = r.w
        dr = wf.Drawer(w, sc, np.random.default_rng(197))
        r.do("wait_load", dict(node=(), group=(), req=None, req_present=None))
        r.do("bound_load", dict(bound=sc["bound"]))
        r.do("nom_load", dr.draw("nom_load", "empty"))
        for cycle in (1, 2, 3):
            gone = w.placed if w.placed is not None else np.zeros(0, np.int64)
            gone = gone[w.own[gone] == wf.NOM_NONE]
            r.do("pods", dict(remove=np.asarray(gone, np.uint32), insert=wf.new_pods(rng, w.S, np.sort(rng.integers(0, w.g, 24)).astype(np.int32))))
            if cycle == 1:
                r.do("pass")
            else:
                assert np.any(w.own != wf.NOM_NONE), f"cycle {cycle}: no nominee is left in the queue"
                out = r.do("pass_nom", dict(priority=dr._prio(np.arange(w.pods.p)), own_id=w.own.copy()), flat=bool(cycle % 2))
                seen["consumed"] += out["consumed"]["n"]
                seen["blocked"] += out["blocked"]
            a = dr.draw("bind", "cycle")
            if a is not None:
                r.do("bind", a)
            r.do("park")
            assert w.unplaced.size, f"cycle {cycle}: every pod found a node"
            a = _preemptors(w, dr)
            if how == "device":
                cg = r.do("commit_gang", dict(a, nominate=True, clear_lower=True), flat=bool(cycle % 2))
                seen["nominated"] += int((cg["nominated_id"] != wf.NOM_NONE).sum())
            else:
                cg = r.do("commit_gang", dict(a, nominate=False, clear_lower=True), flat=bool(cycle % 2))
                has = cg["res"]["node"] >= 0
                r.do("nom_apply", dict(remove=np.zeros(0, np.uint32), pod_index=a["pod_index"][has], node=cg["res"]["node"][has].astype(np.uint32),
                                       priority=a["priority"][has]))
                seen["nominated"] += int(has.sum())
            seen["cleared"] += len(cg["cleared"]["id"])
            seen["victims"] += int(cg["res"]["n_victims"].sum())
            if cycle == 2:
                assert w.nt.id.size, "cycle 2 leaves no row"
                on = int(w.nt.node[0])
                r.do("nodes", dict(ops=[(wf.REMOVE, on), (wf.APPEND, 0)]))
                r.do("bound_nodes")
                r.do("wait_nodes")
                if how == "device":
                    seen["dropped"] += r.do("nom_nodes")["n"]
                else:
                    rows, own = r.ctx.nominated_read(), w.own.copy()
                    kind, index = [k for k, _ in w.pend_n], [i for _, i in w.pend_n]
                    left = nnr.remap_on_the_host(rows, w.nt.n, kind, index, w.S)
                    seen["dropped"] += rows["id"].size - left["id"].size
                    r.do("nom_load", dict(node=left["node"], priority=left["priority"], req=left["req"], req_present=left["req_present"]))
                    live = np.isin(own, left["id"])
                    w.own[live] = np.searchsorted(left["id"], own[live]).astype(np.uint32)      # (fresh id k is the k-th surviving id)
            r.against_fresh()
        q = np.arange(min(w.pods.p, 12), dtype=np.uint32)
        pre = r.do("preempt", dict(pod_index=q, priority=dr._prio(q), protected=np.zeros(w.g, np.uint8)))["res"]
        req, pres = r.ctx.read_node_requests()
        (ids, nodes), dump, tab = r.ctx.read_bound(), r.ctx.bound_dump(), r.ctx.nominated_read()
        held = dict(node_req=req, node_pres=pres, bound_id=ids, bound_node=nodes, wait=r.ctx.wait_read(), nom_rank=np.argsort(np.argsort(tab["id"])),
                    nom={f: tab[f] for f in NOM_COLUMNS[1:]}, bound=dump, preempt=pre)
    print(f"the cycle with nomination ({how}): {seen}")
    return seen, held


def test_the_documented_cycle_with_nomination(bsa, soa, orc):
    """include/bsched.h, the nominated-pod table: the cycle with the table's own device paths and a twin that goes the host way at every point
    where there is one (bs_nominated_apply for NOMINATE's tail; bs_nominated_read, a remap on the host and bs_nominated_load for
    bs_nominated_nodes_apply) hold the same table up to the id map, the same node requests, bound and wait tables, and answer the next
    bs_preempt_run identically.  (The rows a pass under rule S consumes and the rows BS_PREEMPT_CLEAR_LOWER clears leave on the device in both:
    a removal by bs_nominated_apply in their place would need a pass and a plan that do not see them go.)"""
    seen, held = _nominating_cycle(bsa, soa, orc, "device")
    assert seen["nominated"] and seen["consumed"] and seen["dropped"] and seen["victims"], seen
    seen_host, held_host = _nominating_cycle(bsa, soa, orc, "host")
    assert seen_host == seen

    def same(a, b, what):
        if isinstance(a, dict):
            for k in a:
                same(a[k], b[k], f"{what}: {k}")
        else:
            assert np.array_equal(a, b), f"the device paths against the host way: {what}"
    same(held, held_host, "held")


def test_the_documented_cycle_with_the_scored_pass(bsa, soa, orc):
    """the same cycle without a nominated-pod table and with bs_seq_run_scored((1, 0, 1)) as its pass, held against the model call by call;
    after three cycles some gang has been released on nodes first fit would not have used"""
    sc = wf.scene(9)
    rng = np.random.default_rng(299)
    elsewhere = 0
    with Runner(bsa, soa, orc, sc, "the cycle with the scored pass") as r:
        w = r.w
        dr = wf.Drawer(w, sc, np.random.default_rng(297))
        r.do("wait_load", dict(node=(), group=(), req=None, req_present=None))
        r.do("bound_load", dict(bound=sc["bound"]))
        for cycle in (1, 2, 3):
            gone = w.placed if w.placed is not None else np.zeros(0, np.int64)
            r.do("pods", dict(remove=np.asarray(gone, np.uint32), insert=wf.new_pods(rng, w.S, np.sort(rng.integers(0, w.g, 24)).astype(np.int32))))
            first = ssoa.seq_pass(orc, w.nodes(), w.fit(), w.groups, w.pods, w.leader, ssoa.first_fit)
            s = r.do("pass_scored", dict(weights=(1, 0, 1)), flat=bool(cycle % 2))["seq"]
            grouped = (w.pods.group >= 0) & (w.pods.group < w.g)
            rel = grouped & (s["pod_node"] >= 0) & (first["pod_node"] >= 0)        # gang pods that both passes released
            elsewhere += int(np.any(s["pod_node"][rel] != first["pod_node"][rel]))
            a = dr.draw("bind", "cycle")
            if a is not None:
                r.do("bind", a)
            r.do("park")
            if w.unplaced.size:
                r.do("commit_gang", dict(_preemptors(w, dr), assume=True), flat=bool(cycle % 2))
            r.against_fresh()
    assert elsewhere, "no gang is released on nodes first fit would not have used"
