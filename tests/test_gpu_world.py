"""Many cycles on ONE context with every resident table in play, against the composite model of tests/world_ref.py.

The single-feature tests pin each entry point; this module pins what crosses them on the host side of the library (csrc/bs_ctx.hpp): the
count and window guards, the scratch blocks that are "zero between calls" and whose layouts follow N, G and the id spaces, the
pointer-swapped twins of the group pack, the bound table and the wait table, the lazily re-derived queue state.  After EVERY call the
cheap reads (groups, queue, node requests, findMaxPG, the wait table, the bound table with its PDB column, the resident PDBs, the
pass's waiting pods while the window is open, bs_preempt_gang_read, the nominated-pod table with its count and id space, the reports of
the last pass and of the last preemption call) must equal the model bit for bit, every call's own results are
compared field for field with the reference of that call, a predicted refusal must give the status the header names and change
nothing, and every 8th step a context loaded afresh from the model's arrays (ids mapped by table order) must answer bs_preempt_run and,
while no leader is carried, a batch with every stage exactly as the context under test does."""
import numpy as np
import pytest

import groups_list_ref as gl
import preempt_pdb_ref as pp
import world_ref as wf
from test_gpu_parity import assert_batch_equal

pytestmark = pytest.mark.gpu
BOUND_COLUMNS = ("priority", "start_ns", "group", "req", "req_present", "pdb")
NOM_COLUMNS = ("id", "node", "priority", "req", "req_present")
SEQ_FIELDS = ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods", "n_released")


def status_of(bsa, fn):
    try:
        fn()
    except bsa.BsError as e:
        return e.status
    return 0


class Runner:
    """a context and the World beside it: `do` makes one call on both and holds the device against the model"""

    def __init__(self, bsa, soa, orc, sc, tag):
        self.bsa, self.soa, self.orc, self.tag = bsa, soa, orc, tag
        self.w = wf.world_of(orc, sc)
        self.ctx = bsa.Context(scalar_lanes=sc["S"])
        self.ctx.load_nodes(sc["nodes"], sc["fit"])
        self.ctx.load_groups(sc["groups"])
        self.ctx.load_pods(sc["pods"])
        self.log = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def where(self):
        return f"{self.tag} step {len(self.log) - 1} {self.log[-1]} after {self.log[:-1]}"

    # ---- the reads ------------------------------------------------------------------------------------------------------------------
    def check_reads(self):
        ctx, w, bsa, where = self.ctx, self.w, self.bsa, self.where()
        r = w.reads()
        got = ctx.read_groups()
        for name in gl.COLUMNS:
            assert np.array_equal(getattr(got, name), getattr(r["groups"], name)), f"{where}: groups.{name}"
        assert ctx.read_pods().equal(r["pods"]), f"{where}: the queue"
        req, pres = ctx.read_node_requests()
        assert np.array_equal(pres, r["node_pres"]), f"{where}: node request keys"
        bad = np.nonzero(req != r["node_req"])
        assert bad[0].size == 0, f"{where}: node requests differ first at lane {bad[0][:1]} node {bad[1][:1]}: {req[bad][:1]} vs {r['node_req'][bad][:1]}"
        assert ctx.find_max_pg() == r["find_max_pg"], f"{where}: findMaxPG"
        assert (ctx.wait_count(), ctx.wait_ids()) == (r["wait_count"], r["wait_ids"]), f"{where}: wait count, ids"
        if r["wait"] is None:
            assert status_of(bsa, ctx.wait_read) == wf.STATE, f"{where}: bs_wait_read with stale counts"
        else:
            t = ctx.wait_read()
            for name, col in r["wait"].items():
                assert np.array_equal(t[name], col), f"{where}: wait table: {name}"
        if r["bound"] is None:
            assert status_of(bsa, ctx.read_bound) == wf.STATE, f"{where}: bs_bound_read before bs_bound_load"
        else:
            ids, nodes = ctx.read_bound()
            tab = r["bound"]
            assert np.array_equal(ids, tab["id"]) and np.array_equal(nodes, tab["node"]), f"{where}: bs_bound_read"
            dump = ctx.bound_dump()
            for name in BOUND_COLUMNS:
                assert np.array_equal(dump[name], tab[name]), f"{where}: bs_bound_dump: {name}"
            assert ctx.bound_ids() == r["bound_ids"], f"{where}: bs_bound_ids"
        if r["pdb"] is None:
            assert status_of(bsa, ctx.pdb_read) == wf.STATE, f"{where}: bs_pdb_read without resident PDBs or with a stale node count"
        else:
            p = ctx.pdb_read()
            assert (p["n_pdb"], p["covered"]) == (r["pdb"]["n_pdb"], r["pdb"]["covered"]), f"{where}: bs_pdb_read counts"
            assert np.array_equal(p["allowed"], r["pdb"]["allowed"]) and np.array_equal(p["node_violating"], r["pdb"]["node_violating"]), f"{where}: bs_pdb_read"
        if r["waiting"] is None:
            assert status_of(bsa, ctx.seq_waiting_read) == wf.STATE, f"{where}: bs_seq_waiting_read outside the window"
        else:
            assert np.array_equal(ctx.seq_waiting_read(), r["waiting"]), f"{where}: bs_seq_waiting_read"
        if w.gang is not None:                                  # the arrays of the last bs_preempt_commit_gang, under that call's g
            q, g, voided, placed = w.gang
            v, p = self.gang_read(q, g)
            assert np.array_equal(v, voided) and np.array_equal(p, placed), f"{where}: bs_preempt_gang_read"
            if w.g != g:
                assert status_of(bsa, lambda: self.gang_read(q, w.g)) == wf.INVALID, f"{where}: bs_preempt_gang_read with the new g"
        # the nominated-pod table: count and id space from the first load on, the columns while its node count is the list's
        if r["nom_count"] is None:
            assert status_of(bsa, ctx.nominated_count) == wf.STATE and status_of(bsa, ctx.nominated_ids) == wf.STATE, f"{where}: bs_nominated_count before a load"
        else:
            assert (ctx.nominated_count(), ctx.nominated_ids()) == (r["nom_count"], r["nom_ids"]), f"{where}: nominated count, ids"
            if r["nom"] is None:
                assert status_of(bsa, ctx.nominated_read) == wf.STATE, f"{where}: bs_nominated_read with a stale node count"
            else:
                t = ctx.nominated_read()
                for name in NOM_COLUMNS:
                    assert np.array_equal(t[name], r["nom"][name]), f"{where}: nominated table: {name}"
        # the reports of the last pass ...
        if r["seq_nominated"] is None:
            assert status_of(bsa, ctx.seq_nominated_read) == wf.STATE, f"{where}: bs_seq_nominated_read after a pass that is not its own"
        else:
            c = ctx.seq_nominated_read()
            for name in ("n", "id", "pod", "node"):
                assert np.array_equal(c[name], r["seq_nominated"][name]), f"{where}: bs_seq_nominated_read: {name}"
        if r["seq_score"] is None:
            assert status_of(bsa, ctx.seq_score_read) == wf.STATE, f"{where}: bs_seq_score_read after a pass that is not its own"
        else:
            sc = ctx.seq_score_read(p=r["seq_score"]["p"])                       # (readable with that pass's p while it is the last pass)
            assert np.array_equal(sc["total"], r["seq_score"]["total"]) and np.array_equal(sc["n_fit"], r["seq_score"]["n_fit"]), f"{where}: bs_seq_score_read"
            if w.pods.p != r["seq_score"]["p"]:
                assert status_of(bsa, ctx.seq_score_read) == wf.INVALID, f"{where}: bs_seq_score_read with the new queue length"
        # ... and of the last successful preemption call
        if r["pre_nominated"] is None:
            assert status_of(bsa, lambda: ctx.preempt_nominated_read(1)) == wf.STATE, f"{where}: bs_preempt_nominated_read after a call without the flag"
        else:
            assert np.array_equal(ctx.preempt_nominated_read(len(r["pre_nominated"])), r["pre_nominated"]), f"{where}: bs_preempt_nominated_read"
        if r["pre_cleared"] is None:
            assert status_of(bsa, ctx.preempt_cleared_read) == wf.STATE, f"{where}: bs_preempt_cleared_read after a call without the flag"
        else:
            c = ctx.preempt_cleared_read()
            for name in ("id", "node", "priority", "by"):
                assert np.array_equal(c[name], r["pre_cleared"][name]), f"{where}: bs_preempt_cleared_read: {name}"

    def gang_read(self, q, g):
        import ctypes as C
        voided, placed = np.zeros(max(q, 1), np.uint8), np.zeros(max(g, 1), np.uint32)
        self.ctx._chk(self.ctx._lib.bs_preempt_gang_read(self.ctx._h, q, voided.ctypes.data_as(C.POINTER(C.c_uint8)), g,
                                                         placed.ctypes.data_as(C.POINTER(C.c_uint32))), "bs_preempt_gang_read")
        return voided[:q], placed[:g]

    # ---- one call ------------------------------------------------------------------------------------------------------------------
    def do(self, kind, args=None, refused=False, flat=False):
        """the call on the model, then on the device; -> the model's results"""
        args = {} if args is None else args
        self.log.append(("!" if refused else "") + kind)
        exp = self.w.step(kind, args)
        where = self.where()
        assert (exp["status"] != wf.OK) == refused, f"{where}: the model answers {exp['status']}"
        if refused:
            st = status_of(self.bsa, lambda: self.call(kind, args, exp, flat))
            assert st == exp["status"], f"{where}: status {st}, the header says {exp['status']}"
        else:
            self.compare(kind, self.call(kind, args, exp, flat), exp, where)
        self.check_reads()
        return exp

    def call(self, kind, a, exp, flat):
        ctx, soa = self.ctx, self.soa
        if kind == "pods":
            return ctx.apply_pods(remove=a["remove"], insert=a["insert"])
        if kind == "groups":
            return ctx.apply_group_deltas(a["deltas"])
        if kind == "batch":
            ctx.run(a["stages"] | (soa.BATCH_COMMIT if a["commit"] else 0))
            return ctx.read(bitmap=False, rows=False)
        if kind == "pass":
            return ctx.seq_run(soa.STAGE_PREFILTER)
        if kind == "pass_nom":
            return ctx.seq_run_nominated(a["priority"], a["own_id"], stages=soa.STAGE_PREFILTER | (soa.STAGE_FILTER if a.get("filter") else 0), flat=flat)
        if kind == "pass_scored":
            return ctx.seq_run_scored(a["weights"], flat=flat)
        if kind == "nom_load":
            return ctx.nominated_load(a["node"], a["priority"], a["req"], a["req_present"])
        if kind == "nom_apply":
            return dict(first_id=ctx.nominated_apply(a["remove"], a["pod_index"], a["node"], a["priority"]))
        if kind == "nom_nodes":
            ids, nodes, prio, n = ctx.nominated_nodes_apply(exp["kind"], exp["index"])
            return dict(n=n, id=ids, node=nodes, priority=prio)
        if kind == "list":
            return ctx.groups_list_apply(a["remove"], a["update"], a["rows"], a["n_append"], flat=flat)
        if kind == "nodes":
            return ctx.apply_node_deltas(exp["deltas"])
        if kind == "assume":
            return ctx.assume_nodes(a["reqs"])
        if kind == "wait_load":
            return ctx.wait_load(a["node"], a["group"], a["req"], a["req_present"])
        if kind == "park":
            return ctx.wait_park()
        if kind == "release":
            return ctx.wait_release(a["groups"])
        if kind == "expire":
            return ctx.wait_expire(a["groups"], deny=a["deny"])
        if kind == "forget":
            return dict(node=ctx.wait_forget(a["ids"]))
        if kind == "wait_nodes":
            ids, nodes, groups, n = ctx.wait_nodes_apply(exp["kind"], exp["index"])
            return dict(n=n, id=ids, node=nodes, group=groups)
        if kind == "seq_expire":
            return ctx.seq_expire(a["groups"], deny=a["deny"], all=a["all"], flat=flat)
        if kind == "bound_load":
            return ctx.load_bound(a["bound"])
        if kind == "bound_apply":
            return dict(first_id=ctx.bound_apply(a["remove"], a["insert"], a["pdb"], flat=flat))
        if kind == "bound_apply_ex":
            return dict(first_id=ctx.bound_apply_ex(a["remove"], a["insert"], a["pdb"], flags=a.get("flags", 1), flat=flat))
        if kind == "bind":
            return ctx.bound_bind(a["wait_ids"], a["pod_index"], a["priority"], a["start_ns"], a["pdb"])
        if kind == "bound_nodes":
            n, ids = ctx.bound_nodes_apply(exp["kind"], exp["index"], dropped_cap=ctx.bound_count())
            return dict(n_dropped=n, dropped=ids)
        if kind == "pdb_set":
            return ctx.bound_pdb_set(a["bits"])
        if kind == "pdb_load":
            return ctx.pdb_load(a["allowed"], a["off"], a["member"])
        if kind == "pdb_append":
            return ctx.pdb_members_append(exp["first_id"], a["off"], a["member"])
        if kind == "pdb_allowed":
            return ctx.pdb_allowed_apply(a["index"], a["value"])
        if kind == "preempt":
            return dict(res=ctx.preempt(a["pod_index"], a["priority"], a["protected"], victim_cap=wf.CAP))
        if kind == "commit":
            return dict(res=ctx.preempt_commit(a["pod_index"], a["priority"], a["protected"], victim_cap=wf.CAP, apply=a["apply"], assume=a["assume"],
                                               nominate=a.get("nominate", False), clear_lower=a.get("clear_lower", False)))
        if kind == "commit_gang":
            return dict(res=ctx.preempt_commit_gang(a["pod_index"], a["priority"], a["protected"], gang_need=a["need"], victim_cap=wf.CAP, apply=a["apply"],
                                                    assume=a["assume"], flat=flat, nominate=a.get("nominate", False), clear_lower=a.get("clear_lower", False)))
        raise KeyError(kind)

    def compare(self, kind, got, exp, where):
        same = lambda names, g=None, e=None: [self._eq((got if g is None else g)[f], (exp if e is None else e)[f], f"{where}: {f}") for f in names]
        if kind == "batch":
            assert_batch_equal(got, exp["batch"], where, bitmap=False)
        elif kind in ("pass", "pass_nom", "pass_scored"):
            same(SEQ_FIELDS, e=exp["seq"])
            if kind == "pass_nom":
                same(("n", "id", "pod", "node"), g=self.ctx.seq_nominated_read(), e=exp["consumed"])
            if kind == "pass_scored":
                same(("total", "n_fit"), g=self.ctx.seq_score_read())
        elif kind == "nom_apply":
            same(("first_id",))
        elif kind == "nom_nodes":
            same(("n", "id", "node", "priority"))
        elif kind == "list":
            same(("g_new", "n_pods_missing", "n_bound_missing", "n_wait_dropped", "wait_id", "wait_node", "wait_group"))
        elif kind == "park":
            same(("first_id", "n", "pod", "node"))
        elif kind == "release":
            same(("n", "id", "node", "group_entries"))
        elif kind == "expire":
            same(("n", "id", "node", "group_entries", "group_unknown"))
        elif kind == "forget":
            same(("node",))
        elif kind == "wait_nodes":
            same(("n", "id", "node", "group"))
        elif kind == "seq_expire":
            same(("n_groups", "n_pods", "group", "group_pods", "group_earlier", "pod", "node"))
        elif kind in ("bound_apply", "bound_apply_ex"):
            same(("first_id",))
        elif kind == "bind":
            same(("first_id", "node"))
        elif kind == "bound_nodes":
            same(("n_dropped", "dropped"))
        elif kind in ("preempt", "commit", "commit_gang"):
            same(pp.FIELDS, g=got["res"], e=exp["res"])
            if kind == "commit_gang":
                same(("slot_voided", "group_placed"), g=got["res"])
            if "nominated_id" in exp:
                same(("nominated_id",), g=got["res"])
            if "cleared" in exp:
                same(("id", "node", "priority", "by"), g=got["res"]["cleared"], e=exp["cleared"])

    @staticmethod
    def _eq(a, b, what):
        assert np.array_equal(np.asarray(a), np.asarray(b)), f"{what}: {np.asarray(a).tolist()} vs {np.asarray(b).tolist()}"

    # ---- a context loaded afresh from the model's arrays ------------------------------------------------------------------------------
    def against_fresh(self):
        """bs_preempt_run and, while no leader is carried, a batch with every stage: this context and one loaded afresh"""
        w, soa, where = self.w, self.soa, f"{self.where()}: against a context loaded afresh"
        if w.pend_w or w.pend_b or w.pend_n:
            return
        f = w.fresh_arrays()
        with self.bsa.Context(scalar_lanes=w.S) as b:
            b.load_nodes(f["nodes"], f["fit"])
            b.load_groups(f["groups"])
            b.load_pods(f["pods"])
            if f["wait"] is not None:
                t = f["wait"]
                b.wait_load(t["node"], t["group"], t["req"], t["req_present"])
                tb = b.wait_read()
                assert np.array_equal(f["wait_keep"][tb["id"]] if tb["id"].size else tb["id"], t["id"]), f"{where}: wait ids through the map"
                for name in ("node", "group", "req", "req_present"):
                    assert np.array_equal(tb[name], t[name]), f"{where}: wait table: {name}"
            if f["nom"] is not None:                                # (before the preemption call below: rule N on both sides)
                t = f["nom"]
                b.nominated_load(t["node"], t["priority"], t["req"], t["req_present"])
                tb = b.nominated_read()
                assert np.array_equal(f["nom_keep"][tb["id"]] if tb["id"].size else tb["id"], t["id"]), f"{where}: nominated ids through the map"
                for name in NOM_COLUMNS[1:]:
                    assert np.array_equal(tb[name], t[name]), f"{where}: nominated table: {name}"
            if f["bound"] is not None:
                keep = f["bound_keep"]
                b.load_bound(f["bound"])
                b.bound_pdb_set(f["bound_bits"])
                (ia, na), (ib, nb) = self.ctx.read_bound(), b.read_bound()
                assert np.array_equal(keep[ib] if ib.size else ib, ia) and np.array_equal(na, nb), f"{where}: the bound table through the id map"
                da, db = self.ctx.bound_dump(), b.bound_dump()
                for name in BOUND_COLUMNS:
                    assert np.array_equal(da[name], db[name]), f"{where}: bound column {name}"
                if w.preempt_ok() == wf.OK and w.pods.p:
                    q = np.arange(min(w.pods.p, 12), dtype=np.uint32)
                    prio = np.full(q.size, 350, np.int32)
                    prot = (np.arange(w.g) % 5 == 0).astype(np.uint8)
                    ra, rb = self.ctx.preempt(q, prio, prot, victim_cap=wf.CAP), wf.map_victims(b.preempt(q, prio, prot, victim_cap=wf.CAP), keep)
                    for name in pp.FIELDS:
                        assert np.array_equal(ra[name], rb[name]), f"{where}: bs_preempt_run: {name}"
                    w.gang = w.pre_nom = w.pre_clr = None      # (the context's last preemption call is this one now)
            if w.leader < 0 and w.pods.p:
                ra, rb = self.ctx.batch(soa.STAGE_ALL, bitmap=True), b.batch(soa.STAGE_ALL, bitmap=True)
                assert_batch_equal(ra, rb, f"{where}: batch", bitmap=False)
                assert np.array_equal(ra.fl_bitmap, rb.fl_bitmap), f"{where}: batch: Filter bitmap"


@pytest.mark.parametrize("seed", range(wf.SEEDS))
def test_many_cycles_on_one_context(seed, bsa, soa, orc):
    sc, steps = wf.plan(seed, orc)
    with Runner(bsa, soa, orc, sc, f"seed {seed}") as r:
        for i, (kind, args, refused) in enumerate(steps):
            r.do(kind, args, refused, flat=bool(i % 2))
            if i % 8 == 7 or i == len(steps) - 1:
                r.against_fresh()


# ---- the header's cycle, scripted --------------------------------------------------------------------------------------------------------
def _gang_preemptors(w, cap=12):
    """the pods the last pass left without a node, each gang one run, and what each gang still needs (at most what it sends)"""
    idx = w.unplaced[:cap]
    grp = w.pods.group[idx]
    prio = np.full(idx.size, 5000, np.int32)
    o = wf.capi.gang_order(grp, prio)
    idx, grp = idx[o], grp[o]
    waiting = np.bincount(w.wt.group, minlength=w.g)[: w.g]
    need = np.minimum(wf.capi.gang_need(w.groups, waiting), np.bincount(grp, minlength=w.g)[: w.g]).astype(np.uint32)
    return dict(pod_index=idx.astype(np.uint32), priority=prio, protected=np.zeros(w.g, np.uint8), need=need, apply=True, assume=True)


def _bind(w, rng):
    """the pods the last pass released, as bound entries on the nodes they were assumed on (their requests are on the nodes already)"""
    s, p = w.last, w.pods
    idx = np.nonzero(s["pod_node"] >= 0)[0]
    ins = wf.soa.Bound(s["pod_node"][idx].astype(np.uint32), rng.choice(wf.BOUND_PRIO, idx.size).astype(np.int32), rng.integers(50, 99, idx.size).astype(np.int64),
                       p.group[idx].copy(), p.req[:, idx].copy(), p.req_present[idx].copy())
    return dict(remove=np.zeros(0, np.uint32), insert=ins, pdb=None, flags=0)


def _cycle_bind(w, dr, rng, row_rng):
    """the header's bind: the lists are the drawer's ("cycle": every wait row of a gang the pass released, every pod it placed); the pods'
    priorities and starts are drawn as _bind draws them, the rows' from a stream of their own, so that the old way can bind the same"""
    a = dr.draw("bind", "cycle")
    assert a is not None, "the pass placed nobody"
    wl, pl = np.sort(a["wait_ids"]), np.sort(a["pod_index"])
    pods = _bind(w, rng)["insert"]
    assert np.array_equal(pl, np.nonzero(w.last["pod_node"] >= 0)[0])
    prio = np.concatenate([row_rng.choice(wf.BOUND_PRIO, wl.size).astype(np.int32), pods.priority])
    start = np.concatenate([row_rng.choice(wf.BIND_START, wl.size).astype(np.int64), pods.start_ns])
    wl = row_rng.permutation(wl).astype(np.uint32)                               # (not ascending: the table's order is not the call's)
    return dict(wait_ids=wl, pod_index=pl.astype(np.uint32), priority=prio, start_ns=start, pdb=None)


def _documented_cycle(bsa, soa, orc, how):
    """three cycles on one context; -> (seen, what the context holds at the end: the bound table through its id map, the wait table, the
    node requests).  how: "apply_ex" binds the placed pods through bs_bound_apply_ex(flags 0) after bs_wait_release and bs_wait_park;
    "bind" follows the header: bs_bound_bind takes the released gangs' wait rows and the placed pods, then bs_wait_park; "old_way" is
    "apply_ex" with the released gangs' wait rows marshalled through the host as well, which is what bs_bound_bind replaced."""
    sc = wf.scene(9)
    rng, row_rng = np.random.default_rng(99), np.random.default_rng(98)
    seen = dict(parked=0, released=0, bound=0, victims=0, voided=0, rows=0)
    with Runner(bsa, soa, orc, sc, f"the documented cycle ({how})") as r:
        w = r.w
        dr = wf.Drawer(w, sc, np.random.default_rng(97))
        r.do("wait_load", dict(node=(), group=(), req=None, req_present=None))
        r.do("bound_load", dict(bound=sc["bound"]))
        for cycle in (1, 2, 3):
            gone = w.placed if w.placed is not None else np.zeros(0, np.int64)
            arrive = np.sort(rng.integers(0, w.g, 24)).astype(np.int32)
            r.do("pods", dict(remove=np.asarray(gone, np.uint32), insert=wf.new_pods(rng, w.S, arrive)))
            s = r.do("pass")["seq"]
            if how == "bind":
                a = _cycle_bind(w, dr, rng, row_rng)
                r.do("bind", a, flat=bool(cycle % 2))
                seen["bound"] += a["pod_index"].size
                seen["rows"] += a["wait_ids"].size
                pk = r.do("park", flat=bool(cycle % 2))
            else:
                a = _cycle_bind(w, dr, rng, row_rng) if how == "old_way" else None    # (before the release: the rows are still there)
                rows = wf.bbr.rows(w.wt, a["wait_ids"], w.pods, s["pod_node"], (), w.S) if a is not None else None
                r.do("release", dict(groups=[int(x) for x in s["released_group"]]))
                pk = r.do("park", flat=bool(cycle % 2))
                if how == "old_way":
                    n = a["wait_ids"].size
                    bind = _bind(w, np.random.default_rng(0))
                    p = bind["insert"]
                    bind["insert"] = soa.Bound(np.concatenate([rows[0], p.node]), a["priority"], a["start_ns"], np.concatenate([rows[1], p.group]),
                                               np.concatenate([rows[2], p.req], axis=1), np.concatenate([rows[3], p.req_present]))
                    seen["rows"] += n
                else:
                    bind = _bind(w, rng)
                r.do("bound_apply_ex", bind, flat=bool(cycle % 2))
                seen["bound"] += bind["insert"].b - (a["wait_ids"].size if a is not None else 0)
            seen["parked"] += pk["n"]
            seen["released"] += int(s["n_released"])
            assert w.unplaced.size, f"cycle {cycle}: every pod found a node"
            cg = r.do("commit_gang", _gang_preemptors(w), flat=bool(cycle % 2))
            seen["victims"] += int(cg["res"]["n_victims"].sum())
            seen["voided"] += int(cg["slot_voided"].sum())
            if cycle == 1:
                assert s["n_released"], "cycle 1 releases no gang"
                r.do("list", dict(remove=[int(s["released_group"][0])], update=[], rows=wf.new_group_rows(rng, w.S, 1), n_append=1))
            if cycle == 2:
                on = int(w.wt.node[0])                                          # a node that holds wait rows (and bound entries) leaves
                r.do("nodes", dict(ops=[(wf.REMOVE, on), (wf.APPEND, 0)]))
                dropped = r.do("bound_nodes")
                lost = r.do("wait_nodes")
                assert dropped["n_dropped"] and lost["n"], "the removed node was empty"
            if cycle == 3:
                oldest = int(w.wt.group[0])
                ex = r.do("expire", dict(groups=[oldest], deny=True))
                assert ex["n"] > 0 and w.groups.flags[oldest] & soa.GROUP_DENIED
            r.against_fresh()
        (ids, nodes), dump, req = r.ctx.read_bound(), r.ctx.bound_dump(), r.ctx.read_node_requests()
        o = np.argsort(ids, kind="stable")                                      # (fresh id k is the k-th smallest id: id_map_by_table_order)
        assert np.array_equal(ids[o], wf.id_map_by_table_order(w.bt.id))
        held = dict(bound_node=nodes[o], wait=r.ctx.wait_read(), node_req=req[0], node_pres=req[1], wait_ids=r.ctx.wait_ids(),
                    **{f"bound_{f}": dump[f][..., o] for f in BOUND_COLUMNS})
        # ... and in table order, ids included: both forms insert the same rows in the same order, so the order inside a node (importance, ties) is the same too
        held["table"] = dict(id=ids, node=nodes, **{f: dump[f] for f in BOUND_COLUMNS})
    print(f"the documented cycle ({how}): {seen}")
    return seen, held


@pytest.mark.parametrize("how", ["apply_ex", "bind"])
def test_the_documented_cycle_with_binding(how, bsa, soa, orc):
    """include/bsched.h: bs_pods_apply -> bs_seq_run -> bind -> bs_preempt_commit_gang(APPLY | ASSUME) for the pods without a node; three cycles on
    one context.  "apply_ex": bs_wait_release(released_group) -> bs_wait_park -> bs_bound_apply_ex (flags 0: the pass assumed these pods
    already).  "bind": bs_bound_bind (the released gangs' wait rows and the placed pods; no release, the rows leave with the bind) ->
    bs_wait_park.  Between cycles 1 and 2 a finished gang leaves the cache and one arrives; between 2 and 3 a node leaves and one arrives,
    and both tables follow; in cycle 3 the gang that has waited longest times out.  After the third cycle the context that bound through
    bs_bound_bind and one that bound the same rows and pods the old way (bs_wait_release, bs_bound_apply_ex) hold the same bound table up to
    ids, the same wait table and the same node requests."""
    seen, held = _documented_cycle(bsa, soa, orc, how)
    assert seen["parked"] >= 3 and seen["released"] and seen["bound"] and seen["victims"], seen
    if how == "bind":
        assert seen["rows"], "no wait row of a released gang was bound"
        seen_old, held_old = _documented_cycle(bsa, soa, orc, "old_way")
        assert seen_old == seen
        for k, v in held.items():
            if isinstance(v, dict):
                for f, col in v.items():
                    assert np.array_equal(col, held_old[k][f]), f"bind against the old way: {k}: {f}"
            else:
                assert np.array_equal(v, held_old[k]), f"bind against the old way: {k}"


# ---- sizes where the scans and copies change shape, reached by calls ---------------------------------------------------------------------------
def test_tables_cross_their_block_edges_mid_sequence(bsa, soa, orc):
    """a wait table loaded with 1023 rows grows past 1024 AND past its quarter of headroom in one park (the twin is allocated again and the
    rows are copied), g goes 255 -> 257 -> 255, a list delta that removes groups brings the table back below 1024 rows, the bound table
    outgrows its headroom in one bs_bound_apply_ex and is compacted by a commit; then bs_bound_bind crosses the same edges
    (_binds_across_the_edges)"""
    from test_gpu_seq_expire import waiting_scene
    G, N, S = 255, 16, 1
    rng = np.random.default_rng(1023)
    nodes, fit, groups, pods = waiting_scene(soa, [2] * G, n_nodes=N, S=S, pods_cap=110, interleave=True, seed=1023)
    bound = wf.new_bound(rng, S, 200, N, G)
    bound.group[:] = np.where(bound.group < 0, 0, bound.group)
    req, pres = wf.ba.stored(bound, S)
    for l in range(4 + S):
        np.add.at(nodes.requested[l], bound.node, req[l])
    np.bitwise_or.at(nodes.requested_present, bound.node, pres)
    nodes.allocatable[3] = nodes.requested[3] + 110
    nodes.allocatable[0] = nodes.requested[0] + 6000                            # room for every queue pod; the preemptors below ask for more than is left
    sc = dict(S=S, nodes=nodes, fit=fit, groups=groups, pods=pods, bound=bound)
    with Runner(bsa, soa, orc, sc, "block edges") as r:
        w = r.w
        rows = wf.new_pods(rng, S, rng.integers(0, G, 1023))
        r.do("wait_load", dict(node=rng.integers(0, N, 1023).astype(np.uint32), group=rows.group, req=rows.req, req_present=rows.req_present))
        r.do("bound_load", dict(bound=bound))
        # the three scratch blocks that are zero between calls get their first size: marks for 1023 ids and 255 groups, sums for 16 nodes
        r.do("forget", dict(ids=np.array([3, 1000], np.uint32)))
        r.do("expire", dict(groups=[7, 200], deny=False))
        r.do("pass")
        pk = r.do("park")
        assert pk["n"] == 510 and w.wt.w > 1023 + 1023 // 4 and w.wt.ids == 1533, "the park stays inside the table's headroom"
        r.do("forget", dict(ids=np.array([5, 1500, 1279], np.uint32)))            # 1533 ids: the marks by id are allocated again
        r.do("list", dict(remove=[], update=[], rows=wf.new_group_rows(rng, S, 2), n_append=2), flat=True)
        assert w.g == 257
        r.do("expire", dict(groups=[256, 0, 128], deny=True))                   # the per-group marks under the new G
        r.do("list", dict(remove=[3, 255], update=[], rows=wf.new_group_rows(rng, S, 0), n_append=0))
        assert w.g == 255
        ins = wf.new_bound(rng, S, 100, N, w.g)
        ins.group[:] = np.where(ins.group < 0, 1, ins.group)
        r.do("bound_apply_ex", dict(remove=w.bt.id[:3].astype(np.uint32), insert=ins, pdb=rng.integers(0, 2, 100).astype(np.uint8)))
        assert w.bt.count == 297 > 200 + 200 // 4, "the delta stays inside the bound table's headroom"
        big = wf.new_pods(rng, S, np.full(6, soa.POD_NOT_GROUPED))                # six pods that fit nowhere until bound pods leave
        big.cls[:] = 0
        big.req[0] = int((w.nl.alloc[0] - w.nl.req[0]).max()) + 20 + 5 * np.arange(6)
        r.do("pods", dict(remove=np.zeros(0, np.uint32), insert=big))
        idx = np.arange(w.pods.p - 6, w.pods.p, dtype=np.uint32)
        cm = r.do("commit", dict(pod_index=idx, priority=np.full(6, 5000, np.int32), protected=np.zeros(w.g, np.uint8), apply=True, assume=False))
        assert int(cm["res"]["n_victims"].sum()) >= 6 and w.bt.count <= 297 - 6, "the commit compacts nothing"
        out = r.do("list", dict(remove=list(range(10, 110)), update=[5], rows=wf.new_group_rows(rng, S, 1), n_append=0), flat=True)
        assert w.g == 155 and w.wt.w < 1024 and out["n_wait_dropped"] > 500
        r.do("release", dict(groups=[154, 0]))
        r.do("list", dict(remove=[], update=[], rows=wf.new_group_rows(rng, S, 170), n_append=170))
        r.do("nodes", dict(ops=[(wf.APPEND, k % N) for k in range(48)]))
        r.do("wait_nodes")
        r.do("bound_nodes")
        assert (w.g, w.n) == (325, 64)
        ex = r.do("expire", dict(groups=[324, 20, 0, 100], deny=True))            # 325 groups, 64 nodes: the marks by group and the sums are allocated again
        assert ex["n"] > 0
        r.do("forget", dict(ids=w.wt.id[[0, -1]].astype(np.uint32)))
        r.against_fresh()
        _binds_across_the_edges(r, sc, rng)


def _binds_across_the_edges(r, sc, rng):
    """bs_bound_bind at the same edges, in one window: the marks by id were allocated for 1533 ids with a quarter of headroom, the bound
    table's twin for the 297 entries of the bs_bound_apply_ex above with a quarter of headroom.  A bind of wait rows uses the marks as they
    are; the park of the same window takes bs_wait_ids past their allocation and the table past 1024 rows; the second bind of the window
    lists the youngest row, so the marks are allocated again inside it; the third takes the wait table below 1024 rows and the bound
    table past its headroom, so the twin is allocated again inside it."""
    w = r.w
    dr = wf.Drawer(w, sc, rng)
    # (wait_room: no earlier allocation of the marks is larger.  The twin is reserved in bytes, padded columns and per-node words included, with
    # a quarter on top: in entries that is about 297 + 297 // 4, so the third bind is held to twice the 297, well past any rounding)
    marks, twin = w.wt.ids + w.wt.ids // 4, 2 * 297
    assert w.wt.ids == 1533 and w.wt.w < 1024 and w.bt.count <= 297
    r.do("pods", dict(remove=np.arange(w.pods.p, dtype=np.uint32), insert=wf.new_pods(rng, w.S, np.repeat(np.arange(320, dtype=np.int32), 2), cls_max=1)))
    r.do("pass")
    free = rng.permutation(np.nonzero(w.last["pod_node"] >= 0)[0])
    assert free.size >= 12 and int((w.wait_node >= 0).sum()) > marks - w.wt.ids, "the pass releases some gangs and leaves more pods waiting than the marks have room for"
    r.do("bind", dr._bind_args(rng.permutation(w.wt.id)[:5], free[:4]))
    pk = r.do("park")
    assert w.wt.ids > marks and w.wt.w > 1024 and w.wt.ids < (1 << 24), "the park takes the ids past the marks' allocation and the table past 1024 rows"
    r.do("bind", dr._bind_args([int(w.wt.id[-1]), int(w.wt.id[0]), pk["first_id"]], free[4:8]), flat=True)
    assert w.bt.count <= 297 + 297 // 8, "the first two binds stay well inside the twin's headroom"
    rows, count = w.wt.w, w.bt.count
    r.do("bind", dr._bind_args(rng.permutation(w.wt.id)[: rows - 1000], free[8:]))
    assert w.wt.w == 1000 < 1024 < rows and w.bt.count > twin > count
    r.do("forget", dict(ids=w.wt.id[[0, -1]].astype(np.uint32)))                   # the marks were left clean, under their new size
    r.do("seq_expire", dict(groups=None, deny=False, all=True))                  # the window is still open: nobody waits in it any more
    r.against_fresh()


def test_a_bind_raises_the_largest_group_the_preemption_calls_check(bsa, soa, orc):
    """include/bsched.h: after bs_bound_bind the largest group index the table is held to name is the maximum of its old value and the
    inserted groups'; the preemption calls answer BS_ERR_INVALID while it is at or above the loaded group count.  While the tables stay
    consistent that value stays below g (a bind's groups are below g, bs_groups_list_apply takes it along), so the fuzz never sees the
    refusal.  Here the table starts empty, so the value is the bind's own maximum m, found on the device: with m + 1 groups (a list delta
    removes the groups above m) the preemption calls run, with a list of m groups loaded they refuse."""
    sc = wf.scene(0)
    assert sc["bound"].b == 0
    with Runner(bsa, soa, orc, sc, "the largest bound group") as r:
        w = r.w
        dr = wf.Drawer(w, sc, np.random.default_rng(3))
        r.do("wait_load", dict(node=(), group=(), req=None, req_present=None))
        r.do("bound_load", dict(bound=sc["bound"]))
        r.do("pass")
        r.do("bind", dr.draw("bind", "cycle"))
        m = w.bound_max
        assert m == int(w.bt.group.max()) and 0 < m < w.g - 1, "the bind names a group, and not the last one"
        r.do("list", dict(remove=list(range(m + 1, w.g)), update=[], rows=wf.new_group_rows(dr.rng, w.S, 0), n_append=0))
        assert (w.g, w.bound_max) == (m + 1, m)
        keep = np.nonzero((w.pods.group >= 0) & (w.pods.group < m))[0][:4]
        r.do("pods", dict(remove=np.setdiff1d(np.arange(w.pods.p), keep).astype(np.uint32), insert=None))
        pre = dict(pod_index=np.arange(keep.size, dtype=np.uint32), priority=np.full(keep.size, 5000, np.int32), protected=np.zeros(w.g, np.uint8))
        r.do("preempt", pre)                                                    # m < g: the call runs
        g = w.groups
        short = soa.Groups(*[np.ascontiguousarray(getattr(g, c)[..., :m]) for c in gl.COLUMNS])
        r.ctx.load_groups(short)                                                # the table names group m, the list ends at m - 1
        for what, fn in [("bs_preempt_run", lambda: r.ctx.preempt(pre["pod_index"], pre["priority"], pre["protected"][:m], victim_cap=wf.CAP)),
                         ("bs_preempt_commit", lambda: r.ctx.preempt_commit(pre["pod_index"], pre["priority"], pre["protected"][:m], victim_cap=wf.CAP, apply=False, assume=False))]:
            assert status_of(bsa, fn) == wf.INVALID, f"{what} with {m} groups while the bound table names group {m}"


def test_a_pod_leaves_a_node_that_lacks_its_scalar_key(bsa, soa, orc):
    """include/bsched.h, bs_seq_expire and bs_wait_expire / bs_wait_forget: a leaving pod whose scalar key the node does not have (a loaded
    row, or a node that bs_nodes_assume rewrote) goes by RemovePod's map rule: the lane counts as 0 before the request is taken off and the
    node's bit becomes set.  Lanes whose key the pod does not have keep word and bit."""
    sc = wf.scene(2)
    S = sc["S"]
    assert S == 2
    rng = np.random.default_rng(11)
    with Runner(bsa, soa, orc, sc, "a key the node lacks") as r:
        w = r.w
        bare = lambda k: dict(reqs=[(int(k), [int(x) for x in w.nl.req[:4, k]] + [77] * S, 0)])     # no key; the words are stale
        r.do("wait_load", dict(node=(), group=(), req=None, req_present=None))
        r.do("assume", bare(0))
        rows = wf.new_pods(rng, S, [0, 1, 1, 2])
        rows.req_present[:] = [1, 3, 2, 0]
        rows.req[4:] = [[5, 6, 0, 0], [0, 7, 8, 0]]
        r.do("wait_load", dict(node=np.zeros(4, np.uint32), group=rows.group, req=rows.req, req_present=rows.req_present))
        r.do("expire", dict(groups=[0, 2], deny=False))                          # key 0 is created; lane 5 keeps its stale word
        assert int(w.nl.rpres[0]) == 1 and w.nl.req[4:, 0].tolist() == [-5, 77]
        r.do("forget", dict(ids=np.array([2, 1], np.uint32)))                   # key 1 is created by two rows at once, key 0 is there now
        assert int(w.nl.rpres[0]) == 3 and w.nl.req[4:, 0].tolist() == [-11, -15]
        # the pass's own pods: a node is rewritten without keys between the pass and bs_seq_expire
        r.do("pass")
        i = int(np.nonzero((w.wait_node >= 0) & (w.pods.req_present != 0))[0][0])
        k, grp = int(w.wait_node[i]), int(w.pods.group[i])
        r.do("assume", bare(k))
        ex = r.do("seq_expire", dict(groups=[grp], deny=False, all=False))
        gone = ex["pod"][ex["node"] == k]
        keys = int(np.bitwise_or.reduce(w.pods.req_present[gone]))
        assert i in gone and int(w.nl.rpres[k]) == keys
        for s in range(S):
            want = -int(w.pods.req[4 + s, gone].sum()) if (keys >> s) & 1 else 77
            assert int(w.nl.req[4 + s, k]) == want, f"lane {4 + s} of node {k}"


def test_gang_read_keeps_the_group_count_of_its_call(bsa, soa, orc):
    """include/bsched.h: bs_preempt_gang_read's arrays are those of the last bs_preempt_commit_gang.  After a bs_groups_list_apply that changes g
    they are read with the g of that call; the new g is BS_ERR_INVALID"""
    sc = wf.scene(9)
    rng = np.random.default_rng(5)
    with Runner(bsa, soa, orc, sc, "gang read") as r:
        w = r.w
        r.do("wait_load", dict(node=(), group=(), req=None, req_present=None))
        r.do("bound_load", dict(bound=sc["bound"]))
        r.do("pass")
        cg = r.do("commit_gang", _gang_preemptors(w))
        q, g_old = len(cg["res"]["node"]), w.g
        assert cg["group_placed"].any()
        r.do("list", dict(remove=[0], update=[], rows=wf.new_group_rows(rng, w.S, 3), n_append=3))
        assert w.g == g_old + 2
        voided, placed = r.gang_read(q, g_old)
        assert np.array_equal(voided, cg["slot_voided"]) and np.array_equal(placed, cg["group_placed"]), "the values of that call, under its g"
        assert status_of(bsa, lambda: r.gang_read(q, w.g)) == wf.INVALID
        assert status_of(bsa, lambda: r.gang_read(q + 1, g_old)) == wf.INVALID
