"""Scenes of bs_nominated_nodes_apply shared by tests/test_nominated_nodes_cpu.py (which verifies on the model that the chosen seeds have
what they are for) and tests/test_gpu_nominated_nodes.py (which replays them on the device).  TEST INFRASTRUCTURE, no GPU: `World` is the
model of everything a context holds that the preemption calls read — the node list (bound_nodes_ref.NodeList), the bound table under
node-list surgery and BS_PREEMPT_APPLY with the device's ids kept beside it, the PDB bits, and the nominated-pod table
(nominated_ref.NomTable under nominated_nodes_ref.nodes_apply) — so that nominated_ref's reference can be asked about the scene as it is NOW."""
import importlib

import numpy as np

import bound_nodes_ref as bn
import nominated_nodes_ref as nn
import nominated_ref as nr
import preempt_gang_scenes as gs
import preempt_pdb_ref as pp

bsa = importlib.import_module("batch-scheduler_amd")
soa = bsa.soa
U, A, R = nn.UPDATE, nn.APPEND, nn.REMOVE
CAP = 8
MODES = ("run", "commit", "gang")


def base_scene(seed, S, gang, n=48, q=24, per_node=(2, 6)):
    """tests/test_gpu_nominated.py's scene at a smaller size: PDB bits, four groups; gang: the preemptors cut into gangs with needs"""
    if gang:
        return gs.gang_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=4, share=0.2)
    sc, bits = pp.pdb_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=4, share=0.2)
    sc["violating"] = bits
    sc["need"] = np.zeros(sc["groups"], np.uint32)
    return sc


def remove_steps(rng, old):
    """(REMOVE, current index) for the OLD nodes `old`, in a random order (valid while no REMOVE of another node comes in between)"""
    gone, steps = [], []
    for k in rng.permutation(sorted(old)):
        steps.append((R, int(k) - sum(x < k for x in gone)))
        gone.append(int(k))
    return steps


class World:
    def __init__(self, sc, rows=None):
        self.sc, self.S = sc, sc["S"]
        self.nl = bn.NodeList(sc["nodes"], sc["fit"])
        b = sc["bound"]
        self.bound = dict(node=b.node.copy(), priority=b.priority.copy(), start_ns=b.start_ns.copy(), group=b.group.copy(), req=b.req.copy(),
                          req_present=b.req_present.copy())
        self.bid = np.arange(b.b, dtype=np.uint32)          # the device's id of every entry the model still holds
        self.bits = np.asarray(sc["violating"], np.uint8).copy()
        self.tab = nr.NomTable(self.S)
        if rows is not None:
            self.tab.load(self.nl.n, rows["node"], rows["priority"], rows["req"], rows["req_present"])

    # -- what the reference is asked about
    def scene(self) -> dict:
        b = self.bound
        return dict(self.sc, nodes=self.nl.nodes(), fit=self.nl.fit(), violating=self.bits.copy(),
                    bound=soa.Bound(b["node"], b["priority"], b["start_ns"], b["group"], b["req"], b["req_present"]))

    def rows(self):
        return self.tab.read() if self.tab.loaded else None

    def expect_raw(self, mode, apply=False, assume=False, rows="table", pick=None) -> dict:
        sc = self.scene()
        pi, pr_ = (sc["pod_index"], sc["priority"]) if pick is None else (sc["pod_index"][pick], sc["priority"][pick])
        rows = self.rows() if isinstance(rows, str) else rows
        prep = pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], sc["violating"])
        a = (prep, sc["fit"], sc["pods"])
        if mode == "run":
            return dict(res=nr.run_nom_np(*a, pi, pr_, sc["protected"], CAP, rows))
        if mode == "commit":
            return nr.commit_nom_np(*a, sc["bound"], pi, pr_, sc["protected"], CAP, rows, apply, assume)
        return nr.gang_nom_np(*a, sc["bound"], pi, pr_, sc["protected"], sc["need"], CAP, rows, apply, assume)

    def mapped(self, exp: dict) -> dict:
        """the reference's answer in the device's ids: victims and the bound table's ids go through self.bid"""
        out = {k: (v if k == "res" else np.array(v, copy=True)) for k, v in exp.items()}
        res = {f: np.array(v, copy=True) for f, v in exp["res"].items()}
        for i in range(len(res["node"])):
            nv = min(int(res["n_victims"][i]), CAP)
            res["victims"][i, :nv] = self.bid[exp["res"]["victims"][i, :nv]]
        out["res"] = res
        if "bound_id" in exp:
            out["bound_id"] = self.bid[exp["bound_id"]] if self.bid.size else np.zeros(0, np.uint32)
        return out

    # -- what changes it
    def cut(self, steps):
        """node-list surgery, steps = [(kind, index)]: the node list and the bound table follow.  -> (deltas, kinds, indices)"""
        n0 = self.nl.n
        deltas = [self.nl.append(int(i) % len(self.nl.pool[1])) if k == A else self.nl.remove(int(i)) if k == R else self.nl.update(int(i))
                  for k, i in steps]
        kinds, idx = [int(d.kind) for d in deltas], [int(d.index) for d in deltas]
        cur = bn.replay(n0, kinds, idx)
        new_of_old = np.full(n0 + 1, -1, np.int64)
        new_of_old[cur[cur >= 0]] = np.nonzero(cur >= 0)[0]
        new = new_of_old[self.bound["node"].astype(np.int64)]
        keep = new >= 0
        self._keep_bound(keep)
        self.bound["node"] = new[keep].astype(np.uint32)
        return deltas, kinds, idx

    def follow(self, kinds, idx) -> dict:
        return nn.nodes_apply(self.tab, kinds, idx, n_expected=self.nl.n)

    def applied(self, exp: dict):
        """BS_PREEMPT_APPLY of the raw reference answer `exp`: the victims leave the bound table, the node requests are exp's"""
        keep = np.zeros(self.bid.size, bool)
        keep[exp["bound_id"]] = True
        self._keep_bound(keep)
        self.nl.req, self.nl.rpres = np.array(exp["req"], np.int64), np.array(exp["pres"], np.uint32)

    def nominate(self, exp: dict, pick=None) -> np.ndarray:
        pi, pr_ = (self.sc["pod_index"], self.sc["priority"]) if pick is None else (self.sc["pod_index"][pick], self.sc["priority"][pick])
        return nr.nominate_rows(self.tab, exp["res"], pi, pr_, self.sc["pods"])

    def _keep_bound(self, keep):
        for f, v in self.bound.items():
            self.bound[f] = v[:, keep] if f == "req" else v[keep]
        self.bid, self.bits = self.bid[keep], self.bits[keep]


def churn_steps(seed, n, rows, removed_with=2, removed_without=2, appended=2):
    """a delta list for a table `rows` on n nodes: `removed_with` nodes that hold rows and `removed_without` that hold none leave (in a
    random order, so that the indices are current ones), `appended` nodes arrive, one node is updated"""
    rng = np.random.default_rng(seed ^ 0x5C7)
    holders = np.unique(rows["node"]).astype(np.int64)
    free = np.setdiff1d(np.arange(n), holders)
    old = list(rng.permutation(holders)[:removed_with]) + list(rng.permutation(free)[:removed_without])
    steps = [(A, int(rng.integers(0, n)))] + remove_steps(rng, old) + [(A, int(rng.integers(0, n))) for _ in range(appended - 1)]
    return steps + [(U, 0)]


# the twins: S -> seed of a gang scene (all three calls are asked on it), picked so that on the model alone the surgery drops a row,
# moves a survivor and leaves rows that change an answer of every mode (tests/test_nominated_nodes_cpu.py asserts all three)
TWIN_SEEDS = {0: 100, 2: 102, 12: 112}


def twin_scene(S, **kw):
    """-> (world before the surgery, steps)"""
    seed = TWIN_SEEDS[S]
    sc = base_scene(seed, S, True)
    rows = nr.nom_rows_for(sc, seed, density=0.6)
    return World(sc, rows), churn_steps(seed, sc["nodes"].n, rows, **kw)


# the fuzz of test 12: seeds picked so that across them at least 20 rows are dropped and every step kind occurs (asserted on the CPU)
FUZZ_SEEDS = tuple(range(300, 320))
FUZZ_KINDS = ("apply", "surgery", "call", "nominate")


def fuzz_plan(seed, steps=12):
    """-> (scene, first rows, [(kind, argument)]): the step list of one fuzz seed, drawn without looking at any state but the counts"""
    rng = np.random.default_rng(seed)
    S = (0, 1, 2)[seed % 3]
    sc = base_scene(seed, S, gang=bool(seed & 1), n=24, q=12)
    rows = nr.nom_rows_for(sc, seed, density=0.5)
    plan = [(FUZZ_KINDS[int(rng.integers(0, 4))], int(rng.integers(0, 1 << 30))) for _ in range(steps)]
    return sc, rows, plan


def fuzz_apply_args(w: World, arg: int):
    """bs_nominated_apply of a fuzz step: up to a third of the rows leave, up to five arrive"""
    rng = np.random.default_rng(arg)
    live = w.tab.id
    remove = rng.permutation(live)[: int(rng.integers(0, live.size // 3 + 1))].astype(np.uint32)
    ni = int(rng.integers(0, 6)) if w.nl.n else 0
    return (remove, rng.integers(0, w.sc["pods"].p, size=ni).astype(np.uint32), rng.integers(0, max(w.nl.n, 1), size=ni).astype(np.uint32),
            rng.integers(0, 6000, size=ni).astype(np.int32))


def fuzz_surgery_steps(w: World, arg: int):
    """node-list surgery of a fuzz step: one or two nodes that hold rows (if any) and one other leave, as many arrive; never below 20 nodes"""
    rng = np.random.default_rng(arg)
    n = w.nl.n
    holders = np.unique(w.tab.node).astype(np.int64)
    old = list(rng.permutation(holders)[: int(rng.integers(1, 3))]) + [int(rng.integers(0, n))]
    old = sorted(set(int(x) for x in old))
    steps = remove_steps(rng, old)
    grow = len(old) + int(rng.integers(-1, 2))
    if n - len(old) + grow < 20:
        grow = 20 - (n - len(old))
    return [(A, int(rng.integers(0, 24))) for _ in range(max(grow, 0))][:1] + steps + [(A, int(rng.integers(0, 24))) for _ in range(max(grow - 1, 0))]


def fuzz_run(seed):
    """the fuzz of one seed on the model, step by step: yields what the device has to be asked and what it has to answer; the world `w`
    of the first item is the state AFTER every later item"""
    sc, rows, plan = fuzz_plan(seed)
    w = World(sc, rows)
    yield ("start", w, rows)
    for kind, arg in plan:
        if kind == "apply":
            args = fuzz_apply_args(w, arg)
            yield ("apply", args, w.tab.apply(*args, sc["pods"]))
        elif kind == "surgery":
            deltas, kinds, idx = w.cut(fuzz_surgery_steps(w, arg))
            yield ("surgery", deltas, kinds, idx, w.follow(kinds, idx))
        elif kind == "call":
            mode = MODES[arg % 3]
            yield ("call", mode, w.mapped(w.expect_raw(mode)))
        else:
            mode = ("commit", "gang")[arg % 2]
            raw = w.expect_raw(mode, True, False)
            exp = w.mapped(raw)
            ids = w.nominate(raw)
            w.applied(raw)
            yield ("nominate", mode, exp, ids)


def appends_scene():
    """24 -> 700 nodes by APPENDs only.  -> (world before the surgery, steps, rows_for): rows_for(world after the surgery) are the
    arguments of a bs_nominated_apply that puts 48 top-priority copies of the queue's largest pod on the appended node the reference
    picks for the first preemptor, and one on node 699 (tests/test_nominated_nodes_cpu.py asserts that they change an answer)"""
    sc = base_scene(61, 2, True, n=24, q=12)
    w = World(sc, nr.nom_rows_for(sc, 61, density=0.5))

    def rows_for(after: World):
        node = int(after.expect_raw("run")["res"]["node"][0])
        pod = int(np.argmax(sc["pods"].req[0]))
        P = int(sc["priority"].max())
        return [], [pod] * 49, [node] * 48 + [699], [P] * 49
    return w, [(A, i % 24) for i in range(676)], rows_for
