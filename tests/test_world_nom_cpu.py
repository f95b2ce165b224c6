"""The second plan family and the model alone, no GPU (tests/world_ref.py, plan_nom): the nominated-pod table, BS_PREEMPT_NOMINATE and
BS_PREEMPT_CLEAR_LOWER, bs_seq_run_nominated and bs_seq_run_scored among the calls of every other resident table.  The eight seeds are drawn
and replayed on a fresh World step by step; what the GPU replay of tests/test_gpu_world_nom.py relies on is asserted here on the model: every
new entry point and every hazard occurs often enough, the passes under rules S and P decide something, the invariants hold after every step,
a predicted refusal changes nothing.  The new refusals are counted by the call that is refused and by its cause (NEW_REFUSALS): a stale node
count on either nominated call, and on each of the three preemption calls where the nominated-pod table with its rows is the only stale table;
an own id that is dead, by what killed it (consumed by a pass, dropped with its node, cleared by a commit, removed, past the id space).

The hazards (counted by `Hazards`, a small state machine per letter; a bs_nominated_load resets those that follow one table):
  n_a  a commit that nominates, a queue delta that keeps the nominee, a pass under rule S that consumes its row, a preemption call
  n_b  a pass under rule S that consumes rows, bs_seq_expire of a gang whose consumed pod waits (the row stays dead), then a park or a bind
  n_c  node-list surgery with rows in the table, the three *_nodes_apply (all six orders over the seeds) with a refused nominated or
       preemption call between them
  n_d  surgery that keeps the node count, with rows, then bs_nominated_nodes_apply
  n_e  a gang commit that nominates and voids a run, then bs_nominated_apply removes an id that call created
  n_f  BS_PREEMPT_CLEAR_LOWER with APPLY clears a row; a pass that names a cleared id as an own id is refused, the next pass runs
  n_g  a scored pass with a leader carried in, then a plain pass and a pass under rule S on what it left; n_g_rev: the scored pass after them
  n_h  a scored pass, a queue delta that changes p (bs_seq_score_read: the new p is refused, the old one readable), a plain pass (refused)
  n_i  bs_groups_list_apply changes G between a nominating commit and a pass under rule S
  n_j  a NOMINATE tail takes the table past 256 rows (the smallest allocation: the twin it writes was laid out for fewer); n_j_nodes: the
       table follows APPENDs only, with rows (its per-node words are laid out for the old count)
  n_k  a pass under rule S with a row that frees room (a negative lane), then one on the same table without such a row"""
import numpy as np
import pytest

import nominated_ref as nr
import preempt_gang_ref as pg
import preempt_pdb_ref as pp
import seq_soa_ref as ssoa
import world_ref as wf
from test_world_cpu import _same
from test_world_cpu import _snapshot as _snapshot_old

SEEDS = list(range(wf.NOM_SEEDS))
HAZARDS = ("n_a", "n_b", "n_c", "n_d", "n_e", "n_f", "n_g", "n_g_rev", "n_h", "n_i", "n_j", "n_j_nodes", "n_k")
NEW_CALLS = ("nom_load", "nom_apply", "nom_nodes", "pass_nom", "pass_scored", "commit+nominate", "commit_gang+nominate", "commit+clear_lower",
             "commit_gang+clear_lower")
PREEMPT_CALLS = ("preempt", "commit", "commit_gang")
# every new refusal by the call that is refused and by its cause: a stale node count on each nominated call, and on each preemption call where
# the nominated-pod table with its rows is the ONLY stale table; an own id that is dead, by what killed it; ...
NEW_REFUSALS = ("stale:pass_nom", "stale:nom_apply", "stale_rows:preempt", "stale_rows:commit", "stale_rows:commit_gang",
                "own:consumed", "own:dropped", "own:cleared", "own:removed", "own:unknown", "own_twice", "remove_dead",
                "before_load:pass_nom", "before_load:nom_apply", "filter")


def _snapshot(w):
    out = _snapshot_old(w)
    out["nom"] = (None if w.nt is None else (w.nt.n, w.nt.ids, w.nt.read()), list(w.pend_n), w.own.copy(), w.last_pass_kind, w.consumed, w.score,
                  w.pre_nom, w.pre_clr)
    return out


def _refusal(w, kind, args, status):
    """which of the new refusals this is, from the state it met (nothing changed); None: one of the first family's"""
    stale = w.nt is not None and w.nt.n != w.n
    if kind in ("pass_nom", "nom_apply") and w.nt is None:
        return f"before_load:{kind}"
    if kind == "pass_nom" and args.get("filter"):
        return "filter"
    if kind in ("pass_nom", "nom_apply") and stale:
        return f"stale:{kind}"
    if kind in PREEMPT_CALLS and stale and w.nt.id.size and w.bound_ok():
        return f"stale_rows:{kind}"
    if kind == "pass_nom" and status == wf.INVALID:
        named = args["own_id"][args["own_id"] != wf.NOM_NONE]
        bad = [int(x) for x in named[~np.isin(named, w.nt.id)]]
        if not bad:
            return "own_twice"
        assert len(bad) == 1, "one cause per refusal"
        return "own:" + (w.died[bad[0]] if bad[0] < w.nt.ids else "unknown")
    if kind == "nom_apply" and status == wf.INVALID:
        return "remove_dead"
    return None


class Hazards:
    def __init__(self):
        self.count = dict.fromkeys(HAZARDS, 0)
        self.orders = set()
        self.reset()

    def reset(self):
        self.a = self.b = self.e = self.f = self.g = self.h = self.i = self.k = 0
        self.c, self.g_last = None, None
        self.b_pods, self.e_ids, self.f_ids = set(), set(), set()

    def see(self, kind, args, refused, before, w, out):
        hit = lambda k: self.count.__setitem__(k, self.count[k] + 1)
        created = out.get("nominated_id", np.zeros(0, np.uint32)) if not refused else np.zeros(0, np.uint32)
        created = created[created != wf.NOM_NONE]
        if refused:
            if self.c is not None and 1 <= len(self.c["seen"]) < 3 and kind in PREEMPT_CALLS + wf.NOM_CALLS:
                self.c["refused"] = True
            if self.f == 1 and kind == "pass_nom" and out["status"] == wf.INVALID and set(int(x) for x in args["own_id"]) & self.f_ids:
                self.f = 2
            return
        if kind == "nom_load":
            self.a = self.b = self.e = self.f = self.i = self.k = 0
            self.c = None
        # n_a
        if kind in PREEMPT_CALLS and self.a == 3:
            hit("n_a")
            self.a = 0
        if kind in ("commit", "commit_gang") and created.size:
            self.a = 1
        elif kind == "pods" and self.a == 1:
            self.a = 2 if np.any(w.own != wf.NOM_NONE) else 0
        elif kind == "pass_nom" and self.a == 2:
            self.a = 3 if out["consumed"]["n"] else 2
        # n_b
        if kind == "pass_nom":
            self.b, self.b_pods = (1, set(int(x) for x in out["consumed"]["pod"])) if out["consumed"]["n"] else (0, set())
        elif not w.window:
            self.b = 0
        elif kind == "seq_expire" and self.b == 1 and self.b_pods & set(int(x) for x in out["pod"]):
            self.b = 2
        elif kind in ("park", "bind") and self.b == 2:
            hit("n_b")
            self.b = 0
        # n_c, n_d, n_j_nodes
        if kind == "nodes" and any(k != wf.UPDATE for k, _ in args["ops"]) and before["rows"]:
            kinds = {k for k, _ in args["ops"] if k != wf.UPDATE}
            self.c = dict(seen=[], refused=False, keeps=w.n == before["n"], appends=kinds == {wf.APPEND})
        elif kind in wf.NODES_APPLY and self.c is not None and kind not in self.c["seen"]:
            self.c["seen"].append(kind)
            if kind == "nom_nodes":
                if self.c["keeps"]:
                    hit("n_d")
                if self.c["appends"]:
                    hit("n_j_nodes")
            if len(self.c["seen"]) == 3:
                self.orders.add(tuple(self.c["seen"]))
                if self.c["refused"]:
                    hit("n_c")
                self.c = None
        # n_e
        if kind == "commit_gang" and args.get("nominate"):
            self.e, self.e_ids = (1, set(int(x) for x in created)) if out["slot_voided"].any() and created.size else (0, set())
        elif kind == "nom_apply" and self.e == 1 and self.e_ids & set(int(x) for x in args["remove"]):
            hit("n_e")
            self.e = 0
        elif kind in PREEMPT_CALLS:
            self.e = 0
        # n_f
        if kind in ("commit", "commit_gang") and args.get("clear_lower") and args["apply"] and len(out["cleared"]["id"]):
            self.f, self.f_ids = 1, set(int(x) for x in out["cleared"]["id"])
        elif kind == "pass_nom" and self.f == 2:
            hit("n_f")
            self.f = 0
        # n_g
        if kind == "pass_scored":
            if self.g_last in ("pass", "pass_nom") and before["leader"] >= 0:
                hit("n_g_rev")
            self.g = 1 if before["leader"] >= 0 else 0
        elif kind in ("pass", "pass_nom") and self.g:
            self.g |= 2 if kind == "pass" else 4
            if self.g == 7:
                hit("n_g")
                self.g = 0
        if kind in ("pass", "pass_nom", "pass_scored"):
            self.g_last = kind
        # n_h
        if kind == "pass_scored":
            self.h = 1
        elif kind == "pods" and self.h == 1:
            self.h = 2 if w.pods.p != before["p"] else 0
        elif kind == "pass" and self.h == 2:
            hit("n_h")
            self.h = 0
        elif kind in ("pass", "pass_nom"):
            self.h = 0
        # n_i
        if kind in ("commit", "commit_gang") and created.size:
            self.i = 1
        elif kind == "list" and self.i == 1 and w.g != before["g"]:
            self.i = 2
        elif kind == "pass_nom" and self.i == 2:
            hit("n_i")
            self.i = 0
        elif kind == "pass_nom":
            self.i = 0
        # n_j.  256 is the smallest allocation of csrc/tu_nominated.hip, nom_reserve: max(rows + rows / 4, 256) rows, laid out for exactly N
        # nodes.  The motif loads 204 rows (an allocation of 256) and applies up to 256, so the NOMINATE tail writes past what the twin it
        # writes was laid out for; any APPEND passes the node layout.  If nom_reserve's rule changes, this boundary and the motif's sizes follow it
        if kind in ("commit", "commit_gang") and created.size and before["rows"] <= 256 < w.nt.id.size:
            hit("n_j")
        # n_k
        if kind == "pass_nom":
            if before["grows"]:
                self.k = 1
            elif self.k == 1:
                hit("n_k")
                self.k = 0


@pytest.fixture(scope="module")
def replayed(orc):
    hz = Hazards()
    seeds = []
    for seed in SEEDS:
        sc, steps = wf.plan_nom(seed, orc)
        assert len(steps) == wf.STEPS
        w = wf.world_of(orc, sc)
        hz.reset()
        calls, refusals, new_refusals = dict.fromkeys(NEW_CALLS, 0), 0, dict.fromkeys(NEW_REFUSALS, 0)
        nom_passes = dict(n=0, live=0, blocked=0, consumed=0)
        scored = dict(n=0, differs=0)
        cleared, n_seen, crossed_with_rows = 0, {w.n}, False
        for i, (kind, args, refused) in enumerate(steps):
            where = f"nom seed {seed} step {i} {kind}"
            rows = 0 if w.nt is None else int(w.nt.id.size)
            before = dict(g=w.g, n=w.n, p=w.pods.p, leader=w.leader, rows=rows, refusal=None,
                          grows=bool(rows and np.any(w.nt.req < 0)))
            if kind == "pass_scored" and not refused:
                first = ssoa.seq_pass(orc, w.nodes(), w.fit(), w.groups, w.pods, w.leader, ssoa.first_fit)
            snap = _snapshot(w) if refused else None
            out = w.step(kind, args)
            assert (out["status"] != wf.OK) == refused, f"{where}: status {out['status']}"
            if refused:
                assert _same(snap, _snapshot(w)), f"{where}: a refused call changed the model"
                refusals += 1
                before["refusal"] = _refusal(w, kind, args, out["status"])
                if before["refusal"]:
                    new_refusals[before["refusal"]] += 1
            else:
                if kind in NEW_CALLS:
                    calls[kind] += 1
                for flag in ("nominate", "clear_lower"):
                    if kind in ("commit", "commit_gang") and args.get(flag):
                        calls[f"{kind}+{flag}"] += 1
                if kind == "pass_nom":
                    nom_passes["n"] += 1
                    nom_passes["live"] += rows > 0
                    nom_passes["blocked"] += out["blocked"]
                    nom_passes["consumed"] += out["consumed"]["n"]
                if kind == "pass_scored":
                    scored["n"] += 1
                    scored["differs"] += not np.array_equal(first["assumed"], out["seq"]["assumed"])
                if kind in ("commit", "commit_gang") and args.get("clear_lower") and args["apply"]:
                    cleared += len(out["cleared"]["id"])
            w.invariants()
            hz.see(kind, args, refused, before, w, out)
            n_seen.add(w.n)
            crossed_with_rows |= kind == "nodes" and before["n"] < 64 <= w.n and rows > 0 and all(k != wf.REMOVE for k, _ in args["ops"])
        seeds.append(dict(seed=seed, S=sc["S"], calls=calls, refusals=refusals, new_refusals=new_refusals, nom_passes=nom_passes, scored=scored,
                          cleared=cleared, n_seen=n_seen, crossed_with_rows=crossed_with_rows, g0=sc["groups"].g, p0=sc["pods"].p))
    tot = lambda key: {k: sum(s[key][k] for s in seeds) for k in seeds[0][key]}
    print("\nnew entry points over all seeds:", tot("calls"))
    print("hazards over all seeds:", hz.count, "orders of the three *_nodes_apply:", sorted(hz.orders))
    print("new refusals over all seeds:", tot("new_refusals"))
    for s in seeds:
        print(f"nom seed {s['seed']}: S={s['S']} n {min(s['n_seen'])}..{max(s['n_seen'])} refusals {s['refusals']} pass_nom {s['nom_passes']} "
              f"pass_scored {s['scored']} cleared {s['cleared']}")
    return dict(seeds=seeds, calls=tot("calls"), hazards=hz, new_refusals=tot("new_refusals"))


def test_the_scenes_are_the_sizes_of_the_first_family(replayed):
    seeds = replayed["seeds"]
    assert {s["S"] for s in seeds} == set(wf.SCALARS)
    for s in seeds:
        assert 24 <= s["g0"] <= 40 and s["p0"] <= 200
    assert any(s["crossed_with_rows"] for s in seeds), "no seed takes its node count up across 64 by APPEND while the table holds rows"


def test_every_new_entry_point_occurs_often_enough(replayed):
    for k, c in replayed["calls"].items():
        assert c >= 4, f"{k} occurs {c} times over all seeds"


def test_every_hazard_occurs_three_times(replayed):
    hz = replayed["hazards"]
    for k, c in hz.count.items():
        assert c >= 3, f"hazard {k} occurs {c} times: {hz.count}"
    assert len(hz.orders) == 6, f"the three *_nodes_apply come in {sorted(hz.orders)} only"


def test_a_sixth_of_the_steps_are_refusals_and_every_new_one_occurs(replayed):
    for s in replayed["seeds"]:
        assert 6 <= s["refusals"] <= 10, f"nom seed {s['seed']}: {s['refusals']} refusals in {wf.STEPS} steps"
    for k, c in replayed["new_refusals"].items():
        assert c >= 2, f"the refusal {k} occurs {c} times: {replayed['new_refusals']}"


def test_the_passes_under_rules_s_and_p_decide_something(replayed):
    seeds = replayed["seeds"]
    n, live = sum(s["nom_passes"]["n"] for s in seeds), sum(s["nom_passes"]["live"] for s in seeds)
    assert 3 * live >= 2 * n, f"{live} of {n} passes under rule S run on a table with live rows"
    for s in seeds:
        assert s["nom_passes"]["blocked"] >= 1, f"nom seed {s['seed']}: no pod is turned away from a node by a row"
        assert s["nom_passes"]["consumed"] >= 1, f"nom seed {s['seed']}: no own row is consumed"
        assert s["cleared"] >= 1, f"nom seed {s['seed']}: no commit clears a row"
    n, differs = sum(s["scored"]["n"] for s in seeds), sum(s["scored"]["differs"] for s in seeds)
    assert 3 * differs >= n, f"{differs} of {n} scored passes place a pod elsewhere than first fit would"


def test_without_rows_rule_n_is_the_plain_reference(orc):
    """World takes the plain references while the table is empty or absent: the *_nom_np forms with no rows equal them"""
    sc = wf.scene(9)
    w = wf.world_of(orc, sc)
    w.step("bound_load", dict(bound=sc["bound"]))
    w.step("pass", {})
    dr = wf.Drawer(w, sc, np.random.default_rng(1))
    a = dr.draw("commit_gang", "apply")
    eq, keep, prep = w._prep()
    args = (prep, w.fit(), w.pods)
    pi, pr, prot = np.asarray(a["pod_index"]), np.asarray(a["priority"]), a["protected"]
    empty = nr.NomTable(w.S)
    empty.load(w.n, [], [], None, None)
    for rows in (None, empty.read()):
        assert _same(nr.run_nom_np(*args, pi, pr, prot, wf.CAP, rows), pp.preempt_pdb_np(*args, pi, pr, prot, wf.CAP))
        assert _same(nr.commit_nom_np(*args, eq, pi, pr, prot, wf.CAP, rows, True, True), pp.commit_pdb_np(*args, eq, pi, pr, prot, wf.CAP, True, True))
        gn, gp = nr.gang_nom_np(*args, eq, pi, pr, prot, a["need"], wf.CAP, rows, True, False), pg.gang_np(*args, eq, pi, pr, prot, a["need"], wf.CAP, True, False)
        assert _same(gn, {k: gp[k] for k in gn})


def test_the_plan_is_a_function_of_the_seed(orc):
    from test_world_cpu import plan_digest
    assert plan_digest(wf.plan_nom(2, orc)[1]) == plan_digest(wf.plan_nom(2, orc)[1])
