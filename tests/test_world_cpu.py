"""The plan and the model alone, no GPU (tests/world_ref.py): the twelve fixed seeds are drawn, replayed on a fresh World step by step, and
what the GPU replay of tests/test_gpu_world.py relies on is asserted here on the model: every row of calls and every hazard pair occurs
often enough, the structural invariants hold after every step, the references stay inside their domains, a predicted refusal changes
nothing.

"Kind" is read as a row of the issue's table (queue, groups, list, nodes, wait, window, bound, pdb, preempt): nine rows, at least 2 per
seed and 30 over all seeds.  (The 26 single entry points cannot each occur 30 times in 12 x 56 steps.)  On top of that every single
entry point must occur at least 4 times over all seeds.  bs_bound_bind has hazard pairs and counts of its own
(test_bind_meets_the_other_tables_often_enough)."""
import copy
import dataclasses
import hashlib

import numpy as np
import pytest

import world_ref as wf

SEEDS = list(range(wf.SEEDS))
HAZARDS = ("a", "b", "c_wait_first", "c_bound_first", "c_refused_between", "d", "e", "f", "g", "h", "leader_moves",
           # bs_bound_bind's cross-call state against the other tables' calls
           "bind_preempt_bind", "bind_in_window_expire", "bind_then_list_then_preempt", "refused_bind_then_wait_call", "bind_then_nodes_follow",
           "bind_uncovered_then_pdb")
PREEMPT_CALLS = ("preempt", "commit", "commit_gang")
BIND_REFUSALS = ("bind_stale", "bind_window", "bind_waits", "bind_dead")


def _snapshot(w):
    """the model's whole state as plain arrays, for "a refusal changes nothing" """
    r = w.reads()
    out = {k: copy.deepcopy(v) for k, v in r.items() if k not in ("groups", "pods")}
    out["groups"], out["pods"] = r["groups"].copy(), r["pods"].copy()
    out["extra"] = (w.leader, w.bound_max, w.window, list(w.pend_w), list(w.pend_b), None if w.wt is None else (w.wt.n, w.wt.g),
                    None if w.bt is None else w.bt.n)
    # what bs_bound_bind reads beyond the reads: the pass's result block, and the live wait ids while the counts are stale (with wait_ids: the dead ones)
    out["bind"] = (None if w.last is None else w.last["pod_node"].copy(), None if w.pass_wait is None else w.pass_wait.copy(),
                   None if w.wt is None else w.wt.id.copy())
    return out


def _bind_refusal(w, args, status):
    """which of the plan's four refused binds this one is, from the state it meets (tests/world_ref.py, Drawer.d_refuse)"""
    if status == wf.STATE:
        stale = w.bt is not None and (w.bt.n != w.n or (w.wt is not None and w.wt.n != w.n))
        return "bind_stale" if stale else "bind_window" if len(args["pod_index"]) and not w.window else None
    if status == wf.INVALID and len(args["wait_ids"]) and w.window:
        if any(w.wait_node[int(p)] >= 0 for p in args["pod_index"]):
            return "bind_waits"
        if not np.all(np.isin(args["wait_ids"], w.wt.id)) and np.any(np.isin(args["wait_ids"], w.wt.id)) and len(args["pod_index"]):
            return "bind_dead"
    return None


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if hasattr(a, "min_member"):
        return all(np.array_equal(getattr(a, c), getattr(b, c)) for c in wf.gl.COLUMNS)
    if hasattr(a, "equal"):
        return a.equal(b)
    return a == b


class Hazards:
    """the hazard pairs as small state machines over the replayed steps; a reload of a table (bs_bound_load, bs_wait_load) resets them"""

    def __init__(self):
        self.count = dict.fromkeys(HAZARDS, 0)
        self.e_kinds = set()
        self.blp_outcome = {wf.OK: 0, wf.INVALID: 0}   # what the preemption call of bind_then_list_then_preempt was predicted to answer
        self.reset()

    def reset(self):
        self.a = self.b = self.f = self.g = self.h = self.lm = 0
        self.bpb = self.bwe = self.blp = self.rbw = self.bnf = self.bup = 0
        self.bnf_seen = set()
        self.c = None                      # after node surgery: the *_nodes_apply calls seen so far
        self.d, self.e = False, None

    def see(self, kind, args, refused, before, w, out):
        hit = lambda k: self.count.__setitem__(k, self.count[k] + 1)
        if refused:
            if self.c is not None and len(self.c) == 1 and kind in wf.WAIT_CALLS + wf.BOUND_CALLS:
                hit("c_refused_between")
            if kind == "bind" and before["bind_refusal"] in ("bind_waits", "bind_dead") and len(args["wait_ids"]):
                self.rbw = 1               # found on the device after the marks by id were set
            if kind in PREEMPT_CALLS and self.blp == 2 and out["status"] == wf.INVALID:
                hit("bind_then_list_then_preempt")
                self.blp_outcome[wf.INVALID] += 1
                self.blp = 0
            return
        if kind in ("bound_load", "wait_load"):
            self.reset()
            return
        # (a) park, a list delta that removes a group with wait rows and bound entries, a gang commit that applies
        if kind == "park":
            self.a = max(self.a, 1)
        elif kind == "list" and self.a >= 1 and before["hot_removed"]:
            self.a = 2
        elif kind == "commit_gang" and self.a == 2 and args["apply"]:
            hit("a")
            self.a = 0
        # (b) pass, commit(APPLY | ASSUME), bs_seq_expire with the window still open
        if kind == "pass":
            self.b = 1
        elif not w.window:
            self.b = 0
        elif kind == "commit" and self.b == 1 and args["apply"] and args["assume"]:
            self.b = 2
        elif kind == "seq_expire" and self.b == 2:
            hit("b")
            self.b = 0
        # (c) APPEND / REMOVE, then both *_nodes_apply, in both orders
        if kind == "nodes" and any(k != wf.UPDATE for k, _ in args["ops"]):
            self.c = [] if self.c is None or len(self.c) == 2 else self.c
        elif kind in ("wait_nodes", "bound_nodes") and self.c is not None and kind not in self.c:
            self.c.append(kind)
            if len(self.c) == 2:
                hit("c_wait_first" if self.c[0] == "wait_nodes" else "c_bound_first")
                self.c = None
        # (d) g changes, then bs_wait_expire / bs_wait_release by group
        if kind == "list" and out["g_new"] != before["g"]:
            self.d = True
        elif kind in ("expire", "release") and self.d:
            hit("d")
            self.d = False
        # (e) the node count grows, then bs_wait_expire / bs_wait_forget / bs_seq_expire
        if kind == "nodes" and w.n > before["n"]:
            self.e = set()                 # the calls seen since the count grew: each counts once per growth
        elif kind in ("expire", "forget", "seq_expire") and self.e is not None and kind not in self.e:
            hit("e")
            self.e.add(kind)
            self.e_kinds.add(kind)
        # (f) batch, an update-only delta, an append-only delta, batch
        if kind == "batch":
            if self.f == 3:
                hit("f")
            self.f = 1
        elif kind == "list":
            only_update = len(args["update"]) and not len(args["remove"]) and not args["n_append"]
            only_append = args["n_append"] and not len(args["remove"]) and not len(args["update"])
            self.f = 2 if self.f == 1 and only_update else 3 if self.f == 2 and only_append else self.f if self.f and (only_update or only_append) else 0
        # (g) commit with APPLY, bs_bound_apply_ex, bs_pdb_allowed_apply, commit
        if kind in ("commit", "commit_gang"):
            if self.g == 3:
                hit("g")
                self.g = 0
            if args["apply"]:
                self.g = 1
        elif kind == "bound_apply_ex" and self.g == 1 and args["insert"] is not None:
            self.g = 2
        elif kind == "pdb_allowed" and self.g == 2:
            self.g = 3
        # (not in the issue's list; a stale carried leader showed in one seed only without it) a group below the leader leaves, so the leader's
        # index moves with its group; then a batch or a pass, whose pf_leader starts from it
        if kind == "list" and 0 <= w.leader != before["leader"]:
            self.lm = 1
        elif kind in ("batch", "pass") and self.lm:
            hit("leader_moves")
            self.lm = 0
        # bind, a preemption call (the scratch buffer bind carves its blocks from), bind; no bound reload between them
        if kind == "bind":
            if self.bpb == 2:
                hit("bind_preempt_bind")
            self.bpb = 1
        elif kind in PREEMPT_CALLS and self.bpb:
            self.bpb = 2
        # a bind with pods, then bs_seq_expire in the window the bind kept open
        if kind == "pass" or not w.window:
            self.bwe = 0
        elif kind == "bind" and len(args["pod_index"]):
            self.bwe = 1
        elif kind == "seq_expire" and self.bwe:
            hit("bind_in_window_expire")
            self.bwe = 0
        # a bind that raises the largest group the bound table is held to name, a list delta that removes a group, a preemption call
        if kind == "bind" and w.bound_max > before["bound_max"]:
            self.blp = 1
        elif kind == "list" and self.blp == 1 and len(args["remove"]):
            self.blp = 2
        elif kind in PREEMPT_CALLS and self.blp == 2:
            hit("bind_then_list_then_preempt")
            self.blp_outcome[wf.OK] += 1
            self.blp = 0
        # a bind the device refused after the marks were set, then a successful call of the wait core
        if kind in ("forget", "release", "expire") and self.rbw:
            hit("refused_bind_then_wait_call")
            self.rbw = 0
        # a bind with wait ids (both twins flipped), node-list surgery, both *_nodes_apply
        if kind == "bind" and len(args["wait_ids"]):
            self.bnf = 1
        elif kind == "nodes" and self.bnf == 1 and any(k != wf.UPDATE for k, _ in args["ops"]):
            self.bnf, self.bnf_seen = 2, set()
        elif kind in ("wait_nodes", "bound_nodes") and self.bnf == 2:
            self.bnf_seen.add(kind)
            if len(self.bnf_seen) == 2:
                hit("bind_then_nodes_follow")
                self.bnf = 0
        # a bind while resident PDBs exist (its ids are not covered), then a recompute
        if kind == "pdb_load":
            self.bup = 0
        elif kind == "bind" and before["pdb_resident"]:
            self.bup = 1
        elif kind in ("pdb_allowed", "pdb_append") and self.bup:
            hit("bind_uncovered_then_pdb")
            self.bup = 0
        # (h) a pass that leaves a leader, the leader's group removed, a batch, a pass
        if kind == "pass":
            if self.h == 3:
                hit("h")
            self.h = 1 if w.leader >= 0 else 0
        elif kind == "list" and self.h == 1 and before["leader"] >= 0 and w.leader < 0:
            self.h = 2
        elif kind == "batch" and self.h == 2:
            self.h = 3


@pytest.fixture(scope="module")
def replayed(orc):
    """every seed drawn and replayed once: per seed the counts, the hazards, and what the steps showed"""
    hz = Hazards()
    seeds = []
    for seed in SEEDS:
        sc, steps = wf.plan(seed, orc)
        assert len(steps) == wf.STEPS
        w = wf.world_of(orc, sc)
        hz.reset()
        kinds, rows, refusals = {}, dict.fromkeys(wf.ROWS, 0), 0
        shared_node = evicted_waiting = False
        n_seen, victims = {w.n}, 0
        binds = dict(ok=0, wait=0, pods=0, both=0, empties_wait=0, from_empty=0, sentinel=0, stale_pods_only=0, **dict.fromkeys(BIND_REFUSALS, 0))
        for i, (kind, args, refused) in enumerate(steps):
            where = f"seed {seed} step {i} {kind}"
            before = dict(g=w.g, n=w.n, leader=w.leader, hot_removed=False, bound_max=w.bound_max, pdb_resident=w.pm is not None, bind_refusal=None)
            if kind == "bind":
                nw, npod = len(args["wait_ids"]), len(args["pod_index"])
                if not refused:
                    binds["ok"] += 1
                    binds["wait"] += nw > 0
                    binds["pods"] += npod > 0
                    binds["both"] += nw > 0 and npod > 0
                    binds["empties_wait"] += nw > 0 and nw == w.wt.w
                    binds["from_empty"] += w.bt.count == 0
                    binds["sentinel"] += bool(npod and np.any(w.pods.group[args["pod_index"]] < 0))
            if kind == "list" and w.wt is not None and w.bt is not None:
                before["hot_removed"] = any(np.any(w.wt.group == x) and np.any(w.bt.group == x) for x in args["remove"])
            snap = _snapshot(w) if refused else None
            out = w.step(kind, args)                                            # (a reference that leaves its domain raises here)
            assert (out["status"] != wf.OK) == refused, f"{where}: status {out['status']}"
            if refused:
                assert _same(snap, _snapshot(w)), f"{where}: a refused call changed the model"
                refusals += 1
                if kind == "bind":                                              # (nothing changed: the state the call met is still there)
                    r = before["bind_refusal"] = _bind_refusal(w, args, out["status"])
                    assert r is not None, f"{where}: a refused bind that is none of {BIND_REFUSALS}"
                    binds[r] += 1
                    binds["stale_pods_only"] += r == "bind_stale" and not len(args["wait_ids"])
            else:
                kinds[kind] = kinds.get(kind, 0) + 1
                rows[wf.ROW_OF[kind]] += 1
            w.invariants()
            hz.see(kind, args, refused, before, w, out)
            n_seen.add(w.n)
            if w.wt is not None and w.wt.w:
                pairs = {(int(a), int(b)) for a, b in zip(w.wt.node, w.wt.group)}
                shared_node |= len(pairs) > len({a for a, _ in pairs})
            if not refused and kind in ("commit", "commit_gang") and args["apply"]:
                victims += int(out["res"]["n_victims"].sum())
                if w.wt is not None and out["victim_groups"].size:
                    evicted_waiting |= bool(np.isin(out["victim_groups"], w.wt.group).any())
        seeds.append(dict(seed=seed, S=sc["S"], kinds=kinds, rows=rows, refusals=refusals, shared_node=shared_node, evicted_waiting=evicted_waiting,
                          n_seen=n_seen, victims=victims, g0=sc["groups"].g, p0=sc["pods"].p, b0=sc["bound"].b, binds=binds))
    total_rows = {r: sum(s["rows"][r] for s in seeds) for r in wf.ROWS}
    total_kinds = {k: sum(s["kinds"].get(k, 0) for s in seeds) for k in wf.ROW_OF}
    print("\nrows over all seeds:", total_rows)
    print("entry points over all seeds:", total_kinds)
    print("hazard pairs over all seeds:", hz.count, "(e) through", sorted(hz.e_kinds))
    total_binds = {k: sum(s["binds"][k] for s in seeds) for k in seeds[0]["binds"]}
    print("binds over all seeds:", total_binds, "per seed:", [s["binds"]["ok"] for s in seeds])
    print("bind_then_list_then_preempt: the preemption call predicted OK / INVALID:", hz.blp_outcome[wf.OK], "/", hz.blp_outcome[wf.INVALID])
    for s in seeds:
        print(f"seed {s['seed']}: S={s['S']} g0={s['g0']} p0={s['p0']} b0={s['b0']} n {min(s['n_seen'])}..{max(s['n_seen'])} refusals {s['refusals']} "
              f"victims {s['victims']} rows {s['rows']}")
    return dict(seeds=seeds, rows=total_rows, kinds=total_kinds, hazards=hz, binds=total_binds)


def test_the_scenes_are_the_sizes_the_issue_names(replayed):
    seeds = replayed["seeds"]
    assert {s["S"] for s in seeds} == {0, 1, 2, 12}
    for s in seeds:
        assert 24 <= s["g0"] <= 40 and s["p0"] <= 200 and 0 <= s["b0"] <= 300
    assert any(min(s["n_seen"]) <= 4 < max(s["n_seen"]) for s in seeds), "no seed takes its node count across 4"
    assert any(min(s["n_seen"]) <= 64 < max(s["n_seen"]) for s in seeds), "no seed takes its node count across 64"
    assert sum(1 for s in seeds if 12 <= min(s["n_seen"]) and max(s["n_seen"]) <= 40) >= 8, "the other seeds stay at 12 - 40 nodes"
    assert {s["b0"] for s in seeds} >= {0, 300}


def test_every_row_of_calls_occurs_often_enough(replayed):
    for s in replayed["seeds"]:
        for row, c in s["rows"].items():
            assert c >= 2, f"seed {s['seed']}: {row} occurs {c} times"
    for row, c in replayed["rows"].items():
        assert c >= 30, f"{row} occurs {c} times over all seeds"
    for k, c in replayed["kinds"].items():
        assert c >= 4, f"entry point {k} occurs {c} times over all seeds"


def test_a_sixth_of_the_steps_are_refusals(replayed):
    for s in replayed["seeds"]:
        assert 6 <= s["refusals"] <= 9, f"seed {s['seed']}: {s['refusals']} refusals in {wf.STEPS} steps"


def test_every_hazard_pair_occurs_three_times(replayed):
    hz = replayed["hazards"]
    for k, c in hz.count.items():
        assert c >= 3, f"hazard pair ({k}) occurs {c} times: {hz.count}"
    assert hz.e_kinds == {"expire", "forget", "seq_expire"}, f"(e) is reached through {hz.e_kinds} only"


def test_bind_meets_the_other_tables_often_enough(replayed):
    """the counts of bs_bound_bind over the twelve seeds.  Of the two outcomes of bind_then_list_then_preempt's preemption call only BS_OK can
    occur in a plan whose tables stay consistent: a bind's rows come from the wait table and the queue, whose group columns are below g, so it
    raises the bound table's largest group to g - 1 at most, and a list delta takes a value below g to g_new - 1 at most
    (groups_list_ref.max_group).  BS_ERR_INVALID would need a bound entry that names a group at or above g, which World.invariants rules out."""
    hz, b = replayed["hazards"], replayed["binds"]
    for s in replayed["seeds"]:
        assert s["binds"]["ok"] >= 1, f"seed {s['seed']}: no successful bind"
    assert b["wait"] >= 8 and b["pods"] >= 8 and b["both"] >= 4, b
    assert b["empties_wait"] >= 1, "no bind empties the wait table"
    assert b["from_empty"] >= 1, "no bind runs from an empty bound table"
    assert b["sentinel"] >= 1, "no bind lists a pod whose group is a sentinel"
    for r in BIND_REFUSALS:
        assert b[r] >= 2, f"the refusal {r} occurs {b[r]} times: {b}"
    assert b["stale_pods_only"] >= 1, "bind_stale never lists pods only"
    assert hz.blp_outcome[wf.OK] >= 1, hz.blp_outcome


def test_gangs_share_nodes_and_a_commit_evicts_beside_a_waiting_pod(replayed):
    for s in replayed["seeds"]:
        assert s["shared_node"], f"seed {s['seed']}: never wait rows of two groups on one node"
    assert any(s["evicted_waiting"] for s in replayed["seeds"]), "no commit evicts a victim that shares its group with a wait row"
    assert sum(s["victims"] for s in replayed["seeds"]) >= 30, "the commits evict next to nothing"


def canonical(v, h):
    """feeds one value of a plan into the hash h: arrays as dtype, shape and bytes; the SoA dataclasses field by field; containers in order"""
    if isinstance(v, np.ndarray):
        h.update(f"A{v.dtype.str}{v.shape}".encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif dataclasses.is_dataclass(v):
        h.update(f"D{type(v).__name__}".encode())
        for f in dataclasses.fields(v):
            h.update(f.name.encode())
            canonical(getattr(v, f.name), h)
    elif isinstance(v, dict):
        h.update(b"{")
        for k in sorted(v):
            h.update(str(k).encode())
            canonical(v[k], h)
        h.update(b"}")
    elif isinstance(v, (list, tuple)):
        h.update(b"[")
        for x in v:
            canonical(x, h)
        h.update(b"]")
    elif isinstance(v, (np.generic,)):
        canonical(v.item(), h)
    else:
        assert v is None or isinstance(v, (bool, int, float, str)), type(v)
        h.update(f"S{type(v).__name__}:{v!r};".encode())


def plan_digest(steps) -> str:
    h = hashlib.sha256()
    for kind, args, refused in steps:
        canonical((kind, args, bool(refused)), h)
    return h.hexdigest()


# plan(seed) for seeds 0..11 as the commit before the nominated-pod table entered the model drew them (SHA-256 of plan_digest)
PLAN_DIGESTS = [
    "237583fb278357c297bb18f08c76a4fe43c4ffce65806367c8c98409539ad2f3",
    "54591158857388dafb516f07494b255cd1ab25f270b8444f0c7af137e1827d09",
    "58a368496c61be51b919502b868b0d40c5865cdcecb84bdd749542122d03a08e",
    "293749213ab5811d4e5218fa5f65577c92e6c8fac8e46d2d66ecc3e26a2e632b",
    "2554d63b81a78ee78527dcdc4233f661da3edbd1dc4ed43d080b0642da670eb0",
    "591f1e8aa05f103407875eb34a8e4ead37533998ccfddb77d97df6db816a76ed",
    "f4e1afb37e39cd1a382681ec2312ae35699bc894f6b411e4e0ce22c42cf7f02c",
    "c40eddd7b78bac2749f655ce220c6c7f9f93382db3c74dc10003ee2ed2989170",
    "d5595fa0ba1cf5f190a18f929543071e40697e54afc5c98a1fd55bad70ec15b4",
    "ea14cec095654ea8575bf7e0a0a921c386764535a19b159710fc017fd9d1a530",
    "2643584965699f0442e0767fc69909a80972a39c14ce941f192f706e99a93995",
    "62cc84b8afa9e0ac302aacf100d910f03dedc24ee0a7f3fc020482bb4b83d305",
]


def test_the_plan_is_a_function_of_the_seed(orc):
    for seed in SEEDS:
        assert plan_digest(wf.plan(seed, orc)[1]) == PLAN_DIGESTS[seed], f"plan({seed}) is not the plan it was"
    a, b = wf.plan(3, orc)[1], wf.plan(3, orc)[1]
    assert [(k, r) for k, _, r in a] == [(k, r) for k, _, r in b]
    assert all(_same({x: v for x, v in s[1].items() if not hasattr(v, "as_struct")}, {x: v for x, v in t[1].items() if not hasattr(v, "as_struct")})
               for s, t in zip(a, b))
