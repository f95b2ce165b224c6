"""One model of everything a context holds (TEST INFRASTRUCTURE): the queue, the group list and the leader, the node list and its requests,
the Permit-wait table, bs_seq_expire's window, the bound-pod table with its ids and PDB bits, the resident PDBs.  `World` adds no arithmetic
of its own: every transition hands the world's arrays to the reference that already states the call (tests/*_ref.py, the oracle) and takes
them back.  What two references would each keep a copy of has ONE home here:

  node requests     World.nl.req / .rpres   (handed to seq_expire_ref.State and bound_apply_nodes_ref.State as views, to the preemption
                                             references as a soa.Nodes over the same arrays)
  group columns     World.groups            (matched and flags are handed to the wait references as views)
  bound group column  World.bt.group        (handed to groups_list_ref.list_apply and taken back; nobody else keeps one)
  wait rows         World.wt                (wait_ref.Table)

`World.step(kind, args)` applies one call and returns what the call returns, or {"status": code} for a call the header refuses (the validity
paragraphs of include/bsched.h: stale counts, the window) — a refused call changes nothing here.  bs_bound_bind is `_bind`:
bound_bind_ref.bind over the bound table, the wait table, the queue and the last pass's results at once.  `plan(seed)` draws scenes and
operation sequences on a World of its own, so that whoever replays the steps on a fresh World (tests/test_world_cpu.py) or on a World
beside a device context (tests/test_gpu_world.py) sees the same sequence.

The nominated-pod table is World.nt (nominated_ref.NomTable) with the caller's pod -> row id map World.own beside it: bs_nominated_load /
_apply / _nodes_apply, BS_PREEMPT_NOMINATE and BS_PREEMPT_CLEAR_LOWER on the two commits (with rows the preemption calls answer by rule N:
nominated_ref, preempt_clear_ref), and the passes under rule S and rule P (seq_soa_ref.seq_pass on the world's own arrays).  `plan` draws
none of these and is pinned by digest (tests/test_world_cpu.py); `plan_nom(seed)` is the second family that does (tests/test_world_nom_cpu.py,
tests/test_gpu_world_nom.py)."""
from __future__ import annotations

import importlib

import numpy as np

import bound_apply_nodes_ref as ban
import bound_apply_ref as ba
import bound_bind_ref as bbr
import bound_nodes_ref as bn
import groups_list_ref as gl
import nominated_nodes_ref as nnr
import nominated_ref as nr
import pdb_resident_ref as pdr
import preempt_clear_ref as pcr
import preempt_gang_ref as pg
import preempt_pdb_ref as pp
import seq_expire_ref as ser
import seq_scored_scenes as sss
import seq_soa_ref as ssoa
import wait_nodes_ref as wnr
import wait_ref as wr

bsa = importlib.import_module("batch-scheduler_amd")
soa, capi = bsa.soa, bsa.capi

OK, INVALID, STATE, CAPACITY = 0, -1, -4, -5
NOM_NONE = nr.NONE
NOM_STATUS = {"BS_ERR_STATE": STATE, "BS_ERR_INVALID": INVALID, "BS_ERR_CAPACITY": CAPACITY}
UPDATE, APPEND, REMOVE = bn.UPDATE, bn.APPEND, bn.REMOVE
CAP = 16                                   # victim_cap of every preemption call
# the rows of the table in the issue ("kinds"), and the entry points of each
ROWS = {
    "queue": ("pods",),
    "groups": ("groups", "batch", "pass"),
    "list": ("list",),
    "nodes": ("nodes", "assume"),
    "wait": ("wait_load", "park", "release", "expire", "forget", "wait_nodes"),
    "window": ("seq_expire",),
    "bound": ("bound_load", "bound_apply", "bound_apply_ex", "bind", "bound_nodes", "pdb_set"),
    "pdb": ("pdb_load", "pdb_append", "pdb_allowed"),
    "preempt": ("preempt", "commit", "commit_gang"),
}
# the rows plan_nom adds (plan's own table stays as it is: plan(seed) is pinned by digest)
NOM_ROWS = dict(ROWS, groups=("groups", "batch", "pass", "pass_nom", "pass_scored"), nominated=("nom_load", "nom_apply", "nom_nodes"))
NOM_ROW_OF = {k: row for row, ks in NOM_ROWS.items() for k in ks}
NOM_CALLS = ("nom_apply", "pass_nom")
ROW_OF = {k: row for row, ks in ROWS.items() for k in ks}
WAIT_CALLS = ("park", "release", "expire", "forget")
BOUND_CALLS = ("bound_apply", "bound_apply_ex", "bind", "pdb_set", "pdb_load", "pdb_append", "pdb_allowed", "preempt", "commit", "commit_gang")


def id_map_by_table_order(ids) -> np.ndarray:
    """the ids of a table loaded afresh with these live rows listed in ascending id: fresh id k is the k-th smallest live id.
    -> keep [count]: keep[fresh id] = this table's id (monotone)"""
    return np.sort(np.asarray(ids, np.int64))


def map_victims(res: dict, keep) -> dict:
    """a preemption result of a table loaded afresh, restated in the ids of the table it was loaded from"""
    out = dict(res)
    cap = res["victims"].shape[1]
    live = np.arange(cap)[None] < np.minimum(res["n_victims"], cap)[:, None]
    out["victims"] = np.where(live, keep[res["victims"]] if len(keep) else 0, 0).astype(np.uint32)
    return out


class World:
    def __init__(self, orc, nodes, fit, groups, pods):
        self.orc = orc
        self.S = nodes.lanes - 4
        self.nl = bn.NodeList(nodes, fit)
        self.groups, self.pods, self.leader = groups.copy(), pods.copy(), -1
        self.wt = None                     # wait_ref.Table
        self.wait_node = None              # the window: per queue pod the node it waits on, or None while the window is shut
        self.bt = None                     # bound_apply_ref.Table
        self.bound_max = -1                # the largest group index the bound table is held to name
        self.pm = None                     # pdb_resident_ref.Model
        self.pend_w, self.pend_b = [], []  # node deltas (kind, index) the wait table / the bound table has not followed yet
        self.gang = None                   # the last successful preemption call, when it was bs_preempt_commit_gang: (q, g, voided, placed)
        self.placed = None                 # queue pods the last pass gave a node (until the queue changes): what a caller binds or parks
        self.unplaced = None               # queue pods that passed PreFilter in the last pass and found no node: the preemptors
        self.last = None                   # the last pass's record, while the queue is the one it ran on
        self.pass_wait = None              # the pass's own wait_node as of the pass (bs_wait_park and bs_seq_expire empty World.wait_node)
        self.nt = None                     # nominated_ref.NomTable
        self.pend_n = []                   # node deltas the nominated-pod table has not followed yet
        self.own = np.full(self.pods.p, NOM_NONE, np.uint32)   # the caller's map: per queue pod the id of the table row that IS the pod
        self.died = {}                     # ... and what it knows of the dead ids: id -> "consumed" | "dropped" | "cleared" | "removed"
        self.last_pass_kind = None         # "plain" | "nominated" | "scored": the context's last successful pass
        self.consumed = None               # bs_seq_nominated_read, while last_pass_kind is "nominated"
        self.score = None                  # (p, total, n_fit) of bs_seq_score_read, while last_pass_kind is "scored"
        self.pre_nom = None                # nominated_id [count] of the last successful preemption call, when it carried BS_PREEMPT_NOMINATE
        self.pre_clr = None                # its cleared rows {id, node, priority, by}, when it carried BS_PREEMPT_CLEAR_LOWER

    # ---- counts and validity, as the header states them -------------------------------------------------------------------------------
    @property
    def n(self) -> int:
        return self.nl.n

    @property
    def g(self) -> int:
        return int(self.groups.g)

    @property
    def window(self) -> bool:
        return self.wait_node is not None

    def wait_ok(self) -> bool:
        return self.wt is not None and self.wt.n == self.n and self.wt.g == self.g

    def bound_ok(self) -> bool:
        return self.bt is not None and self.bt.n == self.n

    def nom_ok(self) -> bool:
        return self.nt is not None and self.nt.n == self.n

    def nom_rows(self):
        """the rows rule N reads (bs_nominated_read's columns), None without a table or with an empty one"""
        return self.nt.read() if self.nt is not None and self.nt.id.size else None

    def preempt_ok(self) -> int:
        if not self.bound_ok() or (self.nom_rows() is not None and not self.nom_ok()):
            return STATE
        return INVALID if self.bound_max >= self.g else OK

    def nodes(self):
        """a soa.Nodes over the world's own arrays (no copy)"""
        return self.nl.nodes()

    def fit(self):
        return self.nl.fit()

    def _st(self):
        """seq_expire_ref.State over the world's own arrays: what the wait references change is changed here"""
        st = object.__new__(ser.State)
        st.requested, st.requested_present = self.nl.req, self.nl.rpres
        st.matched, st.flags = self.groups.matched, self.groups.flags
        st.wait_node = self.wait_node if self.wait_node is not None else np.full(self.pods.p, -1, np.int32)
        return st

    def _bound_state(self):
        """bound_apply_nodes_ref.State over the world's table and node requests"""
        s = object.__new__(ban.State)
        s.S, s.n, s.t, s.req, s.pres = self.S, self.n, self.bt, self.nl.req, self.nl.rpres
        return s

    def _shut(self):
        self.wait_node = None

    def _rows_gone(self, ids, why):
        """the caller's map forgets rows that left the table, and keeps why each id died"""
        self.own[np.isin(self.own, np.asarray(ids, np.uint32))] = NOM_NONE
        self.died.update((int(x), why) for x in ids)

    def _queue_changed(self):
        self._shut()
        self.placed = self.unplaced = self.last = self.pass_wait = None

    def _recompute_bits(self):
        self.bt.pdb = self.pm.bits(self.bt.ids)[self.bt.id.astype(np.int64)].astype(np.uint8)

    # ---- what the cheap reads return ------------------------------------------------------------------------------------------------
    def reads(self) -> dict:
        """everything bs_*_read returns now; a read the header refuses in this state is None"""
        leader, _, panic = self.orc.find_max_pg(self.groups)
        out = dict(groups=self.groups, pods=self.pods, node_req=self.nl.req, node_pres=self.nl.rpres, find_max_pg=(leader, panic),
                   wait=None, wait_count=None, wait_ids=None, bound=None, bound_ids=None, pdb=None,
                   waiting=None if self.wait_node is None else self.wait_node,
                   nom_count=None, nom_ids=None, nom=None, seq_nominated=self.consumed if self.last_pass_kind == "nominated" else None,
                   seq_score=self.score if self.last_pass_kind == "scored" else None, pre_nominated=self.pre_nom, pre_cleared=self.pre_clr)
        if self.nt is not None:
            out["nom_count"], out["nom_ids"] = int(self.nt.id.size), int(self.nt.ids)
            if self.nom_ok():
                out["nom"] = self.nt.read()
        if self.wt is not None:
            out["wait_count"], out["wait_ids"] = self.wt.w, self.wt.ids
            if self.wait_ok():
                out["wait"] = self.wt.columns()
        if self.bt is not None:
            out["bound"], out["bound_ids"] = self.bt.table(), self.bt.ids
            if self.pm is not None and self.bound_ok():
                t = out["bound"]
                nv = np.bincount(t["node"].astype(np.int64), weights=t["pdb"], minlength=self.n).astype(np.uint32)[: self.n]
                out["pdb"] = dict(n_pdb=self.pm.n_pdb, covered=self.pm.covered, allowed=self.pm.allowed, node_violating=nv)
        return out

    def invariants(self):
        """structural invariants that hold after every step"""
        g, n = self.g, self.n
        cols = [("queue", self.pods.group)]
        if self.wt is not None:
            cols.append(("wait", self.wt.group))
            assert np.all(np.diff(self.wt.id.astype(np.int64)) > 0), "wait ids ascend strictly"
            assert self.wt.w == 0 or int(self.wt.id[-1]) < self.wt.ids
            if self.wt.n == n:
                assert np.all(self.wt.node < n), "a wait row names a node >= n"
            assert np.all(self.wt.group >= 0), "a wait row without a group"
        if self.bt is not None:
            cols.append(("bound", self.bt.group))
            assert np.unique(self.bt.id).size == self.bt.count, "bound ids are unique"
            assert self.bt.count == 0 or int(self.bt.id.max()) < self.bt.ids
            if self.bt.n == n:
                assert np.all(self.bt.node < n), "a bound entry names a node >= n"
            assert int(self.bt.group.max(initial=-2)) <= self.bound_max or self.bt.count == 0 or int(self.bt.group.max()) < 0, "bound_max_group bounds the bound column"
        if self.nt is not None:
            assert np.all(np.diff(self.nt.id.astype(np.int64)) > 0), "nominated ids ascend strictly"
            assert self.nt.id.size == 0 or int(self.nt.id[-1]) < self.nt.ids
            assert self.nt.id.size <= nr.NOM_MAX
            if self.nt.n == n:
                assert np.all(self.nt.node < n), "a nominated row names a node >= n"
            assert self.own.size == self.pods.p and np.all(np.isin(self.own[self.own != NOM_NONE], self.nt.id)), "the caller's map names a dead row"
        for name, col in cols:
            col = np.asarray(col, np.int64)
            assert np.all((col < g) & (col >= gl.MISSING)), f"{name}: a group index that is neither a sentinel nor < g"
        if self.wait_node is not None:
            assert self.wait_node.size == self.pods.p and np.all(self.wait_node < n)

    # ---- the calls --------------------------------------------------------------------------------------------------------------------
    def step(self, kind: str, a: dict) -> dict:
        """one call: -> its results with status 0, or {"status": code} and nothing changed"""
        out = getattr(self, "_" + kind)(**a)
        out = {} if out is None else out
        out.setdefault("status", OK)
        return out

    def _pods(self, remove=(), insert=None):
        keep = np.ones(self.pods.p, bool)
        keep[np.asarray(remove, np.int64)] = False
        self.own = np.concatenate([self.own[keep], np.full(insert.p if insert is not None else 0, NOM_NONE, np.uint32)])
        self.pods = self.pods.patched(remove=remove, insert=insert, insert_at=None)
        self._queue_changed()

    def _groups(self, deltas):
        for i, m, s, f in deltas:
            self.groups.matched[i], self.groups.status_scheduled[i], self.groups.flags[i] = m, s, f

    def _batch(self, stages, commit):
        sop = self.orc.Sop(self.orc.Snapshot(self.nodes(), self.fit()), self.groups).carry(self.leader)
        exp = sop.batch(self.pods, stages, bitmap=False)
        if commit:
            self.groups, self.leader = sop.groups, sop.leader
        return dict(batch=exp)

    def _pass(self):
        nodes, fit = self.nodes().copy(), self.fit()
        s = self.orc.seq_replay(nodes, fit, self.groups, self.pods, soa.STAGE_PREFILTER, leader=self.leader)
        wait, _ = ser.waiting_after_pass(nodes, fit, self.groups, self.pods, s)
        return self._after_pass(s, wait, "plain")

    def _after_pass(self, s, wait, kind):
        """what every form of the pass leaves: node requests, group state, leader, the window, the pods a caller binds, parks or preempts for"""
        self.last_pass_kind, self.consumed, self.score = kind, None, None
        self.nl.req, self.nl.rpres = s["nodes"].requested.copy(), s["nodes"].requested_present.copy()
        self.groups, self.leader, self.wait_node = s["groups"], s["leader"], wait
        self.placed = np.nonzero((s["pod_node"] >= 0) | (wait >= 0))[0]
        grouped = (self.pods.group >= 0) & (self.pods.group < self.g)
        self.unplaced = np.nonzero((s["pf_code"] < 16) & (s["pod_node"] < 0) & (wait < 0) & grouped)[0]
        self.last, self.pass_wait = s, wait.copy()
        return dict(seq=s)

    def _pass_nom(self, priority, own_id, filter=False):
        """bs_seq_run_nominated: seq_soa_ref.seq_pass under rule S on the table's rows; the consumed rows leave the table (D6)"""
        if filter:
            return dict(status=INVALID)
        if not self.nom_ok():
            return dict(status=STATE)
        named = np.asarray(own_id, np.uint32)[np.asarray(own_id, np.uint32) != NOM_NONE] if own_id is not None else np.zeros(0, np.uint32)
        if not np.all(np.isin(named, self.nt.id)) or np.unique(named).size != named.size:
            return dict(status=INVALID)
        ch = ssoa.NominatedChoice(self.nt.read(), priority, own_id)
        s = ssoa.seq_pass(self.orc, self.nodes(), self.fit(), self.groups, self.pods, self.leader, ch)
        out = self._after_pass(s, s["wait_node"], "nominated")
        c = sorted(ch.consumed)
        self.consumed = dict(n=len(c), **{f: np.array([x[j] for x in c], np.uint32) for j, f in enumerate(("id", "pod", "node"))})
        self.nt.apply(self.consumed["id"], [], [], [], self.pods, n_now=self.n)
        self._rows_gone(self.consumed["id"], "consumed")
        return dict(out, consumed=self.consumed, blocked=ch.blocked)

    def _pass_scored(self, weights):
        """bs_seq_run_scored: seq_soa_ref.seq_pass under rule P"""
        ch = ssoa.ScoredChoice(weights, self.pods.p)
        s = ssoa.seq_pass(self.orc, self.nodes(), self.fit(), self.groups, self.pods, self.leader, ch)
        out = self._after_pass(s, s["wait_node"], "scored")
        self.score = dict(p=self.pods.p, total=ch.total, n_fit=ch.n_fit)
        return dict(out, total=ch.total, n_fit=ch.n_fit)

    # -- the nominated-pod table
    def _nom_load(self, node, priority, req, req_present):
        self.nt = nr.NomTable(self.S)
        self.nt.load(self.n, node, priority, req, req_present)
        self.pend_n = []
        self.own[:] = NOM_NONE
        self.died = {}

    def _nom_apply(self, remove, pod_index, node, priority):
        if self.nt is None:
            return dict(status=STATE)
        try:
            first = self.nt.apply(remove, pod_index, node, priority, self.pods, n_now=self.n)
        except nr.NomRefused as e:
            return dict(status=NOM_STATUS[e.code])
        self._rows_gone(remove, "removed")
        self.own[np.asarray(pod_index, np.int64)] = first + np.arange(len(pod_index), dtype=np.uint32)
        return dict(first_id=first)

    def _nom_nodes(self):
        kind, index = [k for k, _ in self.pend_n], [i for _, i in self.pend_n]
        if self.nt is None:
            return dict(status=STATE, kind=kind, index=index)
        out = nnr.nodes_apply(self.nt, kind, index, n_expected=self.n)
        self.pend_n = []
        self._rows_gone(out["id"], "dropped")
        return dict(out, kind=kind, index=index)

    def _list(self, remove, update, rows, n_append):
        g = self.g
        code = gl.check(g, remove, update, rows.g, n_append)
        if code != gl.OK:
            return dict(status=INVALID)
        if not len(remove) and not len(update) and not n_append:
            return dict(g_new=g, n_pods_missing=0, n_bound_missing=0, n_wait_dropped=0, wait_id=np.zeros(0, np.uint32), wait_node=np.zeros(0, np.uint32),
                        wait_group=np.zeros(0, np.int32))
        wait = self.wt.columns() if self.wt is not None and self.wt.g == g else None
        m = gl.list_apply(self.groups, remove, update, rows, self.pods.group, None if self.bt is None else self.bt.group, wait, self.leader)
        self.groups, self.leader = m["groups"], m["leader"]
        self.pods.group[:] = m["pod_group"]
        if self.bt is not None:
            self.bt.group = m["bound_group"]
            self.bound_max = gl.max_group(self.bound_max, g, remove)
        if wait is not None:
            t = self.wt
            t.id, t.node, t.group, t.req, t.req_present = (m["wait"][k] for k in ("id", "node", "group", "req", "req_present"))
            t.g = m["g_new"]
        self._shut()
        self.last = self.pass_wait = None  # (its released_group names old indices)
        d = m["dropped"]
        return dict(g_new=m["g_new"], n_pods_missing=m["n_pods_missing"], n_bound_missing=m["n_bound_missing"], n_wait_dropped=len(d[0]),
                    wait_id=d[0], wait_node=d[1], wait_group=d[2])

    def _nodes(self, ops):
        """ops: [(UPDATE, index) | (APPEND, like) | (REMOVE, index)] -> the bs_node_delta list"""
        deltas = [self.nl.update(i) if k == UPDATE else self.nl.append(i) if k == APPEND else self.nl.remove(i) for k, i in ops]
        pairs = [(int(d.kind), int(d.index)) for d in deltas]
        if any(k != UPDATE for k, _ in pairs):
            self._shut()
            self.last = self.pass_wait = None          # (its pod_node names old indices)
        if self.wt is not None:
            self.pend_w += pairs
        if self.bt is not None:
            self.pend_b += pairs
        if self.nt is not None:
            self.pend_n += pairs
        return dict(deltas=deltas)

    def _assume(self, reqs):
        for idx, lanes, pres in reqs:
            self.nl.req[:, idx], self.nl.rpres[idx] = lanes, pres

    # -- the wait table
    def _wait_load(self, node, group, req, req_present):
        self.wt = wr.load(self.n, self.g, self.S, node, group, req, req_present)
        self.pend_w = []

    def _park(self):
        if not self.wait_ok() or not self.window:
            return dict(status=STATE)
        return wr.park(self._st(), self.wt, self.pods)

    def _by_group(self, fn, groups):
        if not self.wait_ok():
            return dict(status=STATE)
        try:
            return fn(groups)
        except wr.WaitError as e:
            return dict(status=e.status)

    def _release(self, groups):
        return self._by_group(lambda gs: wr.release(self.wt, gs, self.n, self.g), groups)

    def _expire(self, groups, deny):
        return self._by_group(lambda gs: wr.expire(self._st(), self.wt, gs, deny=deny), groups)

    def _forget(self, ids):
        return self._by_group(lambda il: dict(node=wr.forget(self._st(), self.wt, il)), ids)

    def _wait_nodes(self):
        kind, index = [k for k, _ in self.pend_w], [i for _, i in self.pend_w]
        if self.wt is None or self.wt.g != self.g:
            return dict(status=STATE, kind=kind, index=index)
        out = wnr.nodes_apply(self.wt, self.groups.matched, kind, index, n_expected=self.n, g=self.g)
        self.pend_w = []
        return dict(out, kind=kind, index=index)

    # -- bs_seq_expire
    def _seq_expire(self, groups, deny, all):
        if not self.window:
            return dict(status=STATE)
        return ser.expire(self._st(), self.pods, groups=groups, deny=deny, all=all)

    # -- the bound table
    def _bound_load(self, bound):
        self.bt = ba.Table(bound, self.S, self.n)
        self.bound_max = int(bound.group.max(initial=-1)) if bound.b else -1
        self.pm, self.pend_b = None, []

    def _bound_delta(self, remove, insert, pdb, flags):
        if not self.bound_ok():
            return dict(status=STATE)
        try:
            first = self._bound_state().apply_ex(remove, insert, pdb, flags)
        except ba.ApplyError as e:
            return dict(status=e.status)
        if insert is not None and insert.b:
            self.bound_max = max(self.bound_max, int(insert.group.max()))
        return dict(first_id=first)

    def _bound_apply(self, remove, insert, pdb):
        return self._bound_delta(remove, insert, pdb, 0)

    def _bound_apply_ex(self, remove, insert, pdb, flags=ban.BOUND_NODES):
        return self._bound_delta(remove, insert, pdb, flags)

    def _bind(self, wait_ids, pod_index, priority, start_ns, pdb):
        """bs_bound_bind: bound_bind_ref.bind over the world's own tables.  Node requests, group words, leader, queue and window stay; the
        resident PDB state stays too, as for an insert of bs_bound_apply (the given bits stand until the next recompute)"""
        s = self.last
        try:
            out = bbr.bind(self.bt, self.wt, self.n, self.g, wait_ids, pod_index, priority, start_ns, pdb, pods=self.pods,
                           pod_node=None if s is None else s["pod_node"], wait_node=self.wait_node, window=self.window)
        except bbr.BindError as e:
            return dict(status=e.status)
        self.bound_max = bbr.max_group(self.bound_max, self.bt.group[self.bt.id >= out["first_id"]])
        return out

    def _bound_nodes(self):
        kind, index = [k for k, _ in self.pend_b], [i for _, i in self.pend_b]
        if self.bt is None:
            return dict(status=STATE, kind=kind, index=index)
        _, dropped, _ = bn.nodes_apply(self.bt, kind, index, n_expected=self.n)
        self.pend_b = []
        return dict(n_dropped=int(dropped.size), dropped=dropped, kind=kind, index=index)

    def _pdb_set(self, bits):
        if self.bt is None:
            return dict(status=STATE)
        self.bt.set_pdb(bits)

    def _pdb_load(self, allowed, off, member):
        if self.bt is None:
            return dict(status=STATE)
        assert len(off) - 1 == self.bt.ids
        self.pm = pdr.Model(allowed, off, member)
        self._recompute_bits()

    def _pdb_append(self, off, member):
        if self.bt is None or self.pm is None:
            return dict(status=STATE)
        first = self.pm.covered
        assert first + len(off) - 1 <= self.bt.ids
        self.pm.append(off, member)
        self._recompute_bits()
        return dict(first_id=first)

    def _pdb_allowed(self, index, value):
        if self.bt is None or self.pm is None:
            return dict(status=STATE)
        self.pm.allowed_apply(index, value)
        self._recompute_bits()

    # -- preemption
    def _prep(self):
        eq, keep, bits = self.bt.equivalent()
        return eq, keep, pp.PdbPrep(self.nodes(), eq, self.S, bits)

    def _preempt(self, pod_index, priority, protected):
        code = self.preempt_ok()
        if code:
            return dict(status=code)
        eq, keep, prep = self._prep()
        self.gang = self.pre_nom = self.pre_clr = None
        rows = self.nom_rows()
        if rows is not None:                                                     # rule N
            return dict(res=map_victims(nr.run_nom_np(prep, self.fit(), self.pods, pod_index, priority, protected, CAP, rows), keep))
        return dict(res=map_victims(pp.preempt_pdb_np(prep, self.fit(), self.pods, pod_index, priority, protected, CAP), keep))

    def _written(self, r, keep, apply):
        """what BS_PREEMPT_APPLY leaves: the node requests and the surviving entries"""
        if apply:
            self.nl.req, self.nl.rpres = r["req"].astype(np.int64), r["pres"].astype(np.uint32)
            self.bt._keep(np.isin(self.bt.id, keep[r["bound_id"].astype(np.int64)] if len(keep) else []))

    def _flags_ok(self, apply, assume, nominate) -> int:
        """BS_PREEMPT_NOMINATE: only with APPLY, never with ASSUME, and on a table that is valid for the node count"""
        if nominate and (not apply or assume):
            return INVALID
        return STATE if nominate and not self.nom_ok() else OK

    def _tails(self, r, pod_index, priority, apply, nominate, clear_lower) -> dict:
        """what the two flags leave: the table after the call (preempt_clear_ref.table_after: ONE rewrite), the ids per preemptor, the report"""
        self.pre_nom = self.pre_clr = None
        out = {}
        cleared = r.get("cleared", pcr.cleared_dict([]))
        if self.nt is not None and (nominate or clear_lower):
            ids = pcr.table_after(self.nt, dict(res=r["res"], cleared=cleared), pod_index, priority, self.pods, apply, nominate)
            if apply:
                self._rows_gone(cleared["id"], "cleared")
        if nominate:
            has = ids != NOM_NONE
            self.own[np.asarray(pod_index, np.int64)[has]] = ids[has]
            self.pre_nom = out["nominated_id"] = ids
        if clear_lower:
            self.pre_clr = out["cleared"] = cleared
        return out

    def _commit(self, pod_index, priority, protected, apply, assume, nominate=False, clear_lower=False):
        code = self.preempt_ok() or self._flags_ok(apply, assume, nominate)
        if code:
            return dict(status=code)
        eq, keep, prep = self._prep()
        rows = self.nom_rows()
        if rows is None:
            r = pp.commit_pdb_np(prep, self.fit(), self.pods, eq, pod_index, priority, protected, CAP, apply, assume)
        elif clear_lower:                                                        # rules N and C
            r = pcr.commit_clear_np(prep, self.fit(), self.pods, eq, pod_index, priority, protected, CAP, rows, apply, assume)
        else:                                                                    # rule N
            r = nr.commit_nom_np(prep, self.fit(), self.pods, eq, pod_index, priority, protected, CAP, rows, apply, assume)
        victims = [int(keep[v]) for i in range(len(pod_index)) for v in r["res"]["victims"][i, : min(int(r["res"]["n_victims"][i]), CAP)]]
        vgroups = self.bt.group[np.isin(self.bt.id, victims)].copy()
        self._written(r, keep, apply)
        self.gang = None
        return dict(res=map_victims(r["res"], keep), victim_groups=vgroups, **self._tails(r, pod_index, priority, apply, nominate, clear_lower))

    def _commit_gang(self, pod_index, priority, protected, need, apply, assume, nominate=False, clear_lower=False):
        code = self.preempt_ok() or self._flags_ok(apply, assume, nominate)
        if code:
            return dict(status=code)
        eq, keep, prep = self._prep()
        rows = self.nom_rows()
        a = (prep, self.fit(), self.pods, eq, np.asarray(pod_index), np.asarray(priority), protected, need, CAP)
        if rows is None:
            r = pg.gang_np(*a, apply, assume)
        elif clear_lower:
            r = pcr.gang_clear_np(*a, rows, apply, assume)
        else:
            r = nr.gang_nom_np(*a, rows, apply, assume)
        victims = [int(keep[v]) for i in range(len(pod_index)) for v in r["res"]["victims"][i, : min(int(r["res"]["n_victims"][i]), CAP)]]
        vgroups = self.bt.group[np.isin(self.bt.id, victims)].copy()
        self._written(r, keep, apply)
        self.gang = (len(pod_index), self.g, r["slot_voided"].copy(), r["group_placed"].copy())
        return dict(res=map_victims(r["res"], keep), slot_voided=r["slot_voided"], group_placed=r["group_placed"], victim_groups=vgroups,
                    **self._tails(r, pod_index, priority, apply, nominate, clear_lower))

    # ---- a context loaded afresh from the model's arrays --------------------------------------------------------------------------------
    def fresh_arrays(self) -> dict:
        """what a second context is loaded with: the bound and wait ids restart, so both come with their id maps (by table order)"""
        out = dict(nodes=self.nodes().copy(), fit=self.fit(), groups=self.groups.copy(), pods=self.pods.copy(), wait=None, bound=None)
        if self.wait_ok():
            out["wait"], out["wait_keep"] = self.wt.columns(), id_map_by_table_order(self.wt.id)
        if self.bound_ok():
            eq, keep, bits = self.bt.equivalent()
            assert np.array_equal(keep, id_map_by_table_order(self.bt.id))
            out["bound"], out["bound_keep"], out["bound_bits"] = eq, keep, bits
        out["nom"] = None
        if self.nom_ok():
            out["nom"], out["nom_keep"] = self.nt.read(), id_map_by_table_order(self.nt.id)
        return out


# ======================================================================================================================================
# scenes
# ======================================================================================================================================
N_START = [5, 63, 12, 40, 17, 33, 24, 13, 38, 29, 21, 36]       # seed 0 crosses 4 nodes downwards, seed 1 crosses 64 upwards
SCALARS = [0, 1, 2, 12]
BOUND_PRIO = np.array([0, 100, 200, 300])
BIND_START = np.array([7, 25, 60])                              # (a loaded entry starts at 0 .. 49: 7 and 25 tie with survivors)


def new_pods(rng, S, groups_of, cls_max=2):
    """queue pods as test_gpu_seq_expire.waiting_scene draws them, for the given group column"""
    group = np.asarray(groups_of, np.int32)
    P, L = group.size, 4 + S
    req = np.zeros((L, P), np.int64)
    req[0] = rng.integers(1, 20, P)
    req[1] = rng.integers(1, 1 << 20, P)
    pres = (rng.integers(0, 1 << S, P) if S else np.zeros(P, np.int64)).astype(np.uint32)
    req[4:] = rng.integers(1, 4, (S, P)) * ((pres[None, :] >> np.arange(S, dtype=np.uint32)[:, None]) & 1)
    return soa.Pods(group, req, pres, rng.integers(0, cls_max, P).astype(np.uint32), np.zeros(P, np.uint64), np.zeros(P, np.uint8))


def new_bound(rng, S, b, n, g, nodes=None):
    """bound entries: mostly grouped (an ungrouped or unknown-group entry of low priority keeps grouped preemptors off its whole node)"""
    grp = rng.integers(0, g, b).astype(np.int32)
    u = rng.random(b)
    grp[u < 0.03] = soa.POD_NOT_GROUPED
    grp[(u >= 0.03) & (u < 0.05)] = soa.POD_GROUP_MISSING
    req = np.zeros((4 + S, b), np.int64)
    req[0], req[1] = rng.integers(1, 50, b), rng.integers(1, 1 << 20, b)
    pres = (rng.integers(0, 1 << S, b) if S else np.zeros(b, np.int64)).astype(np.uint32)
    req[4:] = rng.integers(1, 4, (S, b)) * ((pres[None, :] >> np.arange(S, dtype=np.uint32)[:, None]) & 1)
    node = rng.integers(0, n, b) if nodes is None else np.asarray(nodes)
    return soa.Bound(node.astype(np.uint32), rng.choice(BOUND_PRIO, b).astype(np.int32), rng.integers(0, 50, b).astype(np.int64), grp, req, pres)


def new_group_rows(rng, S, k):
    """group rows as waiting_scene makes them: no captured pod, no MinResources; a quorum of 2 .. 6"""
    rows = soa.Groups.empty(k, 4 + S)
    rows.min_member[:] = rng.integers(2, 7, k)
    return rows


def scene(seed: int) -> dict:
    """a gang scene built like test_gpu_seq_expire.waiting_scene: 24 - 40 gangs of 1 - 6 queue pods (at most 200), nodes whose pods lane
    leaves room for about half of the queue, so a pass leaves pods waiting at Permit AND pods without a node; about a third of the gangs
    can reach their quorum inside one pass.  0 - 300 bound entries whose requests the node requests already count."""
    from test_gpu_seq_expire import waiting_scene
    rng = np.random.default_rng(77000 + seed)
    n, S = N_START[seed % len(N_START)], SCALARS[seed % 4]
    G = int(rng.integers(24, 41))
    lens = rng.integers(1, 7, G)
    while lens.sum() > 200:
        lens[int(rng.integers(0, G))] = 1
    matched0 = rng.integers(0, 2, G)
    nodes, fit, groups, pods = waiting_scene(soa, [int(x) for x in lens], n_nodes=n, S=S, pods_cap=110, interleave=bool(seed % 2),
                                             matched0=[int(x) for x in matched0], seed=77100 + seed)
    full = rng.random(G) < 0.35                                                 # these gangs reach their quorum when every member finds a node
    groups.min_member[full] = (lens + matched0)[full]
    pods.cls[:] = rng.integers(0, 2, pods.p)
    fitb = np.ones((2, n), bool)
    fitb[1] = rng.random(n) < 0.8
    fit = soa.FitMasks.from_bool(fitb)
    b = [0, 300, 120, 40][seed % 4] if seed < 4 else int(rng.integers(0, 301))
    bound = new_bound(rng, S, b, n, G)
    req, pres = ba.stored(bound, S)
    with np.errstate(over="ignore"):
        for l in range(4 + S):
            np.add.at(nodes.requested[l], bound.node, req[l])
        np.bitwise_or.at(nodes.requested_present, bound.node, pres)
    # PreFilter sums every lane over the cluster, a pod needs ONE node: nodes with cpu and no pod slot left beside nodes with pod slots and
    # little cpu keep the sums roomy (gangs pass PreFilter) while first fit runs out of nodes (pods without a node, whose preemption
    # frees a pod slot on a cpu-rich node)
    slots = rng.random(n) < 0.4
    slots[int(rng.integers(0, n))] = True
    slots[int((np.nonzero(slots)[0][0] + 1) % n)] = False
    nodes.allocatable[3] = nodes.requested[3] + np.where(slots, 110, rng.integers(0, 2, n))
    nodes.allocatable[0] = np.where(slots, nodes.requested[0] + (rng.uniform(0.5, 1.5, n) * 6 * pods.p / slots.sum()).astype(np.int64), nodes.allocatable[0])
    return dict(seed=seed, S=S, nodes=nodes, fit=fit, groups=groups, pods=pods, bound=bound, gprio=rng.choice([50, 150, 250, 350, 5000], 64).astype(np.int32))


def world_of(orc, sc) -> World:
    return World(orc, sc["nodes"], sc["fit"], sc["groups"], sc["pods"])


# ======================================================================================================================================
# the plan
# ======================================================================================================================================
STEPS, SEEDS = 56, 12
DEATHS = ("consumed", "dropped", "cleared", "removed", "unknown")                # why an id of the nominated-pod table is dead ("unknown": past the id space)
DEBUG = False
# the hazard pairs of tests/test_world_cpu.py as call sequences; (kind, hint) asks the drawer for a particular shape of the call
MOTIFS = {
    "a": ["pass", "park", ("list", "hot"), ("commit_gang", "apply")],
    "b": ["pods", "pass", ("commit", "assume"), ("seq_expire", "one"), "seq_expire"],
    "c": [("nodes", "shrink"), ("refuse", "bind_stale"), "bound_nodes", ("refuse", "stale_wait"), "wait_nodes", "bound_apply", "pdb_set"],
    "d": [("list", "resize"), ("expire", "any"), ("list", "resize"), "release"],
    "e": [("nodes", "grow"), ("refuse", "bind_stale"), "wait_nodes", ("refuse", "stale_bound"), "bound_nodes", ("expire", "any"), "forget", "pass", ("seq_expire", "one"), "seq_expire"],
    "f": [("batch", "plain"), ("list", "update"), "groups", ("list", "append"), ("batch", "plain")],
    "h": ["pass", ("list", "below"), ("batch", "plain"), ("list", "leader"), ("batch", "commit"), "pods", "pass"],
    # bs_bound_bind between the other tables' calls: its blocks in the preemption calls' scratch while the id space grows; the window it
    # keeps open, both twins flipped, bound_max_group raised and lowered; bound ids the resident PDBs do not cover
    # (the two refusals the kernels find are in the motifs where their state is sure to exist: a dead id after a bind of wait rows, a pod
    # that still waits between a pass and its park; each is made once per seed and is followed by the forget it owes)
    "i": ["pass", ("bind", "both"), ("refuse", "bind_dead"), "preempt", ("bind", "wait"), ("commit", "apply"), ("bind", "pods")],
    "j": [("list", "room"), "pods", "pass", ("bind", "pods"), ("refuse", "bind_waits"), ("seq_expire", "one"), "park", ("bind", "wait"), ("list", "hot"), ("commit_gang", "apply")],
    "k": ["pdb_load", ("bind", "both"), "pdb_allowed", "pdb_append", "preempt"],
}
MOTIF_ORDER = ["c", "e", "f", "h"]                          # (a, b and g are in every seed's first cycle; d comes about by itself)
MOTIF_ORDER_BIND = ["i", "j", "k"]                          # two of each list per seed, in turn
# the first cycle is the header's: pass, preemption for the pods without a node, the released gangs leave Permit and bind, the others park;
# then a gang leaves the cache and the next preemption runs on what all that left behind.  An item that is not applicable is left out
OPENING = ["pass", "pdb_load", ("commit", "assume"), ("seq_expire", "one"), ("release", "released"), ("bound_apply_ex", "bind"), "park", "pdb_allowed",
           ("list", "hot"), ("commit_gang", "apply"), "pods"]
# odd seeds bind in the header's new form: bs_bound_bind takes the released gangs' wait rows with it, so no bs_wait_release goes before it
OPENING_BIND = [x for x in OPENING if x != ("release", "released")]
OPENING_BIND[OPENING_BIND.index(("bound_apply_ex", "bind"))] = ("bind", "cycle")
REFUSALS = ["stale_wait", "stale_bound", "window", "list_order", "forget_dead", "expire_twice", "bind_stale", "bind_window", "bind_waits", "bind_dead"]
ON_DEVICE = ("forget_dead", "expire_twice", "bind_waits", "bind_dead")          # found by the kernels: each once per seed, each followed by a successful call


class Drawer:
    """draws the arguments of one call on the world as it is; None when the call is not applicable now (the plan draws again)"""

    def __init__(self, w: World, sc: dict, rng):
        self.w, self.sc, self.rng = w, sc, rng
        self.serial = 0
        self.taken, self.taken_of = set(), None
        self.owed = None                   # (kind, args) of the successful call a refusal found on the device is followed by
        self.nom = False                   # plan_nom's drawer: commits draw the two nominated-table flags as well
        self.last_out = None               # plan_nom: what the last successful call returned
        self.planned = None                # the arguments of the last commit drawn as a plan only ("plan"), for "clear_same"
        self.turn = dict(stale_bound=0, stale_nom=0, death=0)      # refusals take the three preemption calls, and the causes of a dead id, in turn
        self.death_used = dict.fromkeys(DEATHS, 0)

    def draw(self, kind, hint=None):
        w = self.w
        if (w.pend_w or w.pend_b or w.pend_n) and kind in WAIT_CALLS + BOUND_CALLS + NOM_CALLS + ("list", "wait_load", "bound_load", "nom_load", "seq_expire", "pass", "pass_scored", "pods", "assume"):
            return None                    # between node-list surgery and the *_nodes_apply only those, group patches, batches and refusals
        return getattr(self, "d_" + kind)(hint)

    # -- queue, groups
    def d_pods(self, hint):
        w, rng = self.w, self.rng
        remove = w.placed if w.placed is not None and rng.random() < 0.8 else rng.choice(w.pods.p, min(w.pods.p, int(rng.integers(0, 6))), replace=False)
        remove = np.sort(np.asarray(remove, np.int64))
        if hint == "nominees":             # the pods that own a row of the nominated-pod table stay in the queue
            remove = remove[w.own[remove] == NOM_NONE]
        elif hint == "resize" and remove.size == 0 and w.pods.p:
            remove = np.array([w.pods.p - 1], np.int64)
        k = int(min(rng.integers(4, 30), 200 - (w.pods.p - remove.size)))
        grp = rng.integers(0, w.g, max(k, 0)).astype(np.int32)
        u = rng.random(grp.size)
        grp[u < 0.04] = soa.POD_NOT_GROUPED
        grp[(u >= 0.04) & (u < 0.06)] = soa.POD_GROUP_MISSING
        grp = np.sort(grp)
        if w.bt is not None and -1 <= w.bound_max < w.g - 1:
            # gangs the bound table does not name yet, in front of the other arrivals (first fit runs out of nodes): their bind raises its largest group
            grp[: 4] = np.sort(rng.integers(w.bound_max + 1, w.g, grp[: 4].size))
        return dict(remove=remove.astype(np.uint32), insert=new_pods(rng, w.S, grp) if k > 0 else None)

    def d_groups(self, hint):
        w, rng = self.w, self.rng
        deltas = []
        if rng.random() < 0.5:             # the deny entries' TTL ran out
            return dict(deltas=[(int(i), int(w.groups.matched[i]), int(w.groups.status_scheduled[i]), int(w.groups.flags[i]) & ~soa.GROUP_DENIED)
                                for i in np.nonzero(w.groups.flags & soa.GROUP_DENIED)[0]] or [(0, int(w.groups.matched[0]), int(w.groups.status_scheduled[0]), int(w.groups.flags[0]))])
        for i in rng.choice(w.g, 3, replace=False):
            m = int(rng.integers(0, int(w.groups.min_member[i]) + 2))
            f = (int(w.groups.flags[i]) & 0x16) | int(rng.random() < 0.1) | (soa.GROUP_DENIED * int(rng.random() < 0.2))
            deltas.append((int(i), m, int(w.groups.status_scheduled[i]), f))
        return dict(deltas=deltas)

    def d_batch(self, hint):
        commit = hint == "commit" or (hint is None and self.rng.random() < 0.3)
        return dict(stages=soa.STAGE_ALL, commit=bool(commit))

    def d_pass(self, hint):
        return dict() if self.w.pods.p else None

    def d_list(self, hint):
        w, rng = self.w, self.rng
        g = w.g
        room_down, room_up = g - 24, 40 - g
        remove, update, n_append = [], [], 0
        if hint == "hot":                  # a group with wait rows AND bound entries leaves
            if w.wt is None or w.bt is None:
                return None
            hot = np.intersect1d(w.wt.group, w.bt.group[w.bt.group >= 0])
            if not hot.size:
                return None
            remove = [int(rng.choice(hot))]
            n_append = 1 if room_down < 1 else int(rng.integers(0, 2))
        elif hint == "leader":
            if w.leader < 0:
                return None
            remove, n_append = [int(w.leader)], (1 if room_down < 1 else 0)
        elif hint == "below":              # a group below the leader leaves: the leader the context carries moves down with its group
            if w.leader < 1:
                return None
            remove, n_append = [int(rng.integers(0, w.leader))], (1 if room_down < 1 else 0)
        elif hint == "update":
            update = sorted(rng.choice(g, 2, replace=False).tolist())
        elif hint == "append":
            if room_up < 1:
                return None
            n_append = int(rng.integers(1, min(room_up, 3) + 1))
        elif hint == "room":               # new gangs at the top that no table names yet; at 40 groups one leaves for them
            remove = [] if room_up >= 1 else [int(rng.integers(0, g))]
            n_append = int(rng.integers(1, min(room_up + len(remove), 2) + 1))
        else:                              # "resize" changes g; None is anything
            k = int(rng.integers(0 if hint is None else 1, 4))
            remove = sorted(rng.choice(g, k, replace=False).tolist())
            update = sorted(rng.choice(g, int(rng.integers(0, 3)), replace=False).tolist()) if hint is None else []
            if remove and update and rng.random() < 0.3:
                update = sorted(set(update) | {remove[0]})
            n_append = int(rng.integers(0, 4))
            while g - len(remove) + n_append > 40:
                n_append -= 1
            while g - len(remove) + n_append < 24:
                n_append += 1
            if hint == "resize" and n_append == len(remove):
                n_append += 1 if g - len(remove) + n_append < 40 else -1
        if g - len(remove) + n_append < 24 or g - len(remove) + n_append > 40:
            return None
        return dict(remove=remove, update=update, rows=new_group_rows(rng, w.S, len(update) + n_append), n_append=n_append)

    # -- nodes
    def d_nodes(self, hint):
        w, rng = self.w, self.rng
        n, lo = w.n, 3
        hi = 66 if self.sc["nodes"].n > 60 else 40
        ops = []
        if hint is None:
            hint = str(rng.choice(["shrink", "grow", "update", "swap"]))
        like = lambda: int(rng.integers(0, self.sc["nodes"].n))
        if hint == "grow" and n + 1 <= hi:
            ops = [(APPEND, like()) for _ in range(min(hi - n, 3) if hi > 60 else int(rng.integers(1, min(hi - n, 3) + 1)))]
            if rng.random() < 0.4:
                ops.insert(0, (UPDATE, int(rng.integers(0, n))))
        elif hint == "rows" and n - 1 >= lo and w.nt is not None and w.nt.id.size:
            ops = [(REMOVE, int(rng.choice(w.nt.node)))]
        elif hint == "rows_swap" and w.nt is not None and w.nt.id.size:
            ops = [(REMOVE, int(rng.choice(w.nt.node))), (APPEND, like())]
        elif hint == "shrink" and n - 1 >= lo:
            ops = [(REMOVE, int(rng.integers(0, n)))]
            if n - 2 >= lo and hi <= 60 and rng.random() < 0.5:
                ops.append((REMOVE, int(rng.integers(0, n - 1))))
        elif hint == "swap":
            ops = [(REMOVE, int(rng.integers(0, n))), (APPEND, like())]
        elif hint == "update":
            ops = [(UPDATE, int(rng.integers(0, n))) for _ in range(2)]
        return dict(ops=ops) if ops else None

    def d_assume(self, hint):
        w, rng = self.w, self.rng
        reqs = []
        if hint == "free":                 # pods the tables do not hold ended on half of the nodes: several nodes hold the next pods again
            for k in rng.choice(w.n, max(w.n // 2, min(w.n, 2)), replace=False):
                lanes = w.nl.req[:, k].copy()
                lanes[0] = max(int(lanes[0]) - int(rng.integers(100, 400)), 0)
                lanes[3] = max(int(lanes[3]) - int(rng.integers(3, 12)), 0)
                reqs.append((int(k), [int(x) for x in lanes], int(w.nl.rpres[k])))
            return dict(reqs=reqs)
        for k in rng.choice(w.n, min(3, w.n), replace=False):
            lanes = w.nl.req[:, k].copy()
            lanes[0] = max(int(lanes[0]) + int(rng.integers(-200, 30)), 0)      # pods the table does not hold ended, or started
            lanes[1] += int(rng.integers(0, 1 << 16))
            pres = int(w.nl.rpres[k])
            if w.S and rng.random() < 0.5:
                lanes[4] = (lanes[4] if pres & 1 else 0) + 1
                pres |= 1
            reqs.append((int(k), [int(x) for x in lanes], pres))
        return dict(reqs=reqs)

    # -- the wait table
    def d_wait_load(self, hint):
        w, rng = self.w, self.rng
        k = int(rng.integers(0, 30))
        pods = new_pods(rng, w.S, rng.integers(0, w.g, k))
        return dict(node=rng.integers(0, w.n, k).astype(np.uint32), group=pods.group, req=pods.req, req_present=pods.req_present)

    def d_park(self, hint):
        w = self.w
        return dict() if w.wait_ok() and w.window and np.any(w.wait_node >= 0) else None

    def _wait_groups(self, hint):
        w, rng = self.w, self.rng
        if not w.wait_ok() or not w.wt.w:
            return None
        have = np.unique(w.wt.group)
        gs = rng.permutation(have)[: int(rng.integers(1, 4))].tolist()
        if rng.random() < 0.3:
            gs.append(int(rng.choice(np.setdiff1d(np.arange(w.g), gs))))       # a listed group without rows
        return [int(x) for x in gs]

    def d_release(self, hint):
        w = self.w
        if hint == "released":             # the cycle's call: the gangs the pass released, with or without rows in the table
            if not w.wait_ok() or w.last is None or not w.last["n_released"]:
                return None
            return dict(groups=[int(x) for x in w.last["released_group"]])
        gs = self._wait_groups(hint)
        return None if gs is None else dict(groups=gs)

    def d_expire(self, hint):
        gs = self._wait_groups(hint)
        return None if gs is None else dict(groups=gs, deny=bool(self.rng.random() < 0.5))

    def d_forget(self, hint):
        w, rng = self.w, self.rng
        if not w.wait_ok() or not w.wt.w:
            return None
        return dict(ids=rng.permutation(w.wt.id)[: int(rng.integers(1, 4))].astype(np.uint32))

    def d_wait_nodes(self, hint):
        return dict() if self.w.wt is not None and self.w.pend_w else None

    def d_seq_expire(self, hint):
        w, rng = self.w, self.rng
        if not w.window:
            return None
        if hint == "consumed":
            c = w.consumed["pod"] if w.last_pass_kind == "nominated" else np.zeros(0, np.uint32)
            c = c[w.wait_node[c.astype(np.int64)] >= 0]
            return dict(groups=[int(w.pods.group[int(c[0])])], deny=bool(rng.random() < 0.5), all=False) if c.size else None
        if not np.any(w.wait_node >= 0):   # nobody waits: a listed group is expired all the same (matched = 0); the motifs want more
            return dict(groups=[int(rng.integers(0, w.g))], deny=False, all=False) if hint is None and w.last is not None else None
        if hint is None and rng.random() < 0.15:
            return dict(groups=None, deny=bool(rng.random() < 0.5), all=True)
        have = np.unique(w.pods.group[w.wait_node >= 0])
        return dict(groups=[int(x) for x in rng.permutation(have)[: 1 if hint == "one" else int(rng.integers(1, 4))]], deny=bool(rng.random() < 0.5), all=False)

    # -- the bound table
    def d_bound_load(self, hint):
        w, rng = self.w, self.rng
        if w.bt is None:
            return dict(bound=self.sc["bound"])
        return dict(bound=new_bound(rng, w.S, int(rng.integers(0, 301)), w.n, w.g))

    def _bound_delta(self, hint):
        w, rng = self.w, self.rng
        if not w.bound_ok():
            return None
        live = w.bt.id
        remove = rng.permutation(live)[: int(rng.integers(0, min(live.size, 5) + 1))].astype(np.uint32)
        k = int(rng.integers(1 if hint == "insert" else 0, 9))
        insert, pdb = None, None
        if k:
            insert = new_bound(rng, w.S, k, w.n, w.g)
            pdb = rng.integers(0, 2, k).astype(np.uint8) if rng.random() < 0.5 else None
        if not k and not remove.size:
            return None
        return dict(remove=remove, insert=insert, pdb=pdb)

    def d_bound_apply(self, hint):
        return self._bound_delta(hint)

    def d_bound_apply_ex(self, hint):
        w, rng = self.w, self.rng
        if hint == "bind":                 # the cycle's bind: the pods the last pass released leave Permit and are bound where they sit
            if not w.bound_ok():
                return None
            s = w.last
            idx = np.nonzero(s["pod_node"] >= 0)[0] if s is not None else np.zeros(0, np.int64)
            if not idx.size:
                return self._bound_delta("insert")
            p = w.pods
            ins = soa.Bound(s["pod_node"][idx].astype(np.uint32), rng.choice(BOUND_PRIO, idx.size).astype(np.int32), rng.integers(50, 99, idx.size).astype(np.int64),
                            p.group[idx].copy(), p.req[:, idx].copy(), p.req_present[idx].copy())
            self._take(idx)
            return dict(remove=np.zeros(0, np.uint32), insert=ins, pdb=None)
        return self._bound_delta(hint)

    def _bindable(self):
        """the queue pods a bind may list now: the last pass placed them, they did not wait when the pass ended (a pod the pass left waiting
        and bs_wait_park parked since reads as not waiting: the header's unchecked hazard), and no earlier bind of this window took them"""
        w = self.w
        if not w.window or w.last is None:
            return np.zeros(0, np.int64)
        free = np.nonzero((w.last["pod_node"] >= 0) & (w.pass_wait < 0))[0]
        return np.array([int(p) for p in free if int(p) not in self._taken()], np.int64)

    def _taken(self):
        """the queue pods the binds drawn since the last pass listed (every drawn call is made, and succeeds)"""
        if self.taken_of is not self.w.last:
            self.taken, self.taken_of = set(), self.w.last
        return self.taken

    def _take(self, pods):
        self._taken().update(int(p) for p in pods)

    def _bind_args(self, wl, pl):
        """priorities of the bound table's four, starts from three values (ties with survivors and among the rows), bits half the time"""
        rng = self.rng
        n = len(wl) + len(pl)
        return dict(wait_ids=np.asarray(wl, np.uint32), pod_index=np.asarray(pl, np.uint32), priority=rng.choice(BOUND_PRIO, n).astype(np.int32),
                    start_ns=rng.choice(BIND_START, n).astype(np.int64), pdb=rng.integers(0, 2, n).astype(np.uint8) if rng.random() < 0.5 else None)

    def d_bind(self, hint):
        """"wait": rows of the wait table by id, shuffled; "pods": pods the last pass placed; "both"; "cycle": the header's bind, every wait
        row of a gang the last pass released and every pod it placed.  A hint that asks for rows there are none of takes the other kind"""
        w, rng = self.w, self.rng
        if not w.bound_ok():
            return None
        rows = w.wt.id if w.wait_ok() else np.zeros(0, np.uint32)
        free = self._bindable()
        if hint == "cycle":
            rel = w.last["released_group"] if w.last is not None and w.last["n_released"] else []
            wl = rng.permutation(rows[np.isin(w.wt.group, rel)]) if rows.size else rows
            pl = rng.permutation(free)
        else:
            hint = str(rng.choice(["wait", "pods", "both", "both"])) if hint is None else hint
            kw = rows.size if rng.random() < 0.25 else int(rng.integers(1, min(rows.size, 8) + 1)) if rows.size else 0
            kp = free.size if rng.random() < 0.3 else int(rng.integers(1, min(free.size, 6) + 1)) if free.size else 0
            if hint == "wait" and kw:
                kp = 0
            if hint == "pods" and kp:
                kw = 0
            # rows that raise the largest group the bound table names, and pods without a group, go first: they are few
            rows = rows[np.argsort(w.wt.group <= w.bound_max, kind="stable")] if rows.size else rows
            free = free[np.argsort((w.pods.group[free] >= 0) & (w.pods.group[free] <= w.bound_max), kind="stable")]
            wl, pl = rng.permutation(rows[:kw]), rng.permutation(free[:kp])
        if not len(wl) and not len(pl):
            return None
        self._take(pl)
        return self._bind_args(wl, pl)

    def d_bound_nodes(self, hint):
        return dict() if self.w.bt is not None and self.w.pend_b else None

    def d_pdb_set(self, hint):
        w = self.w
        return dict(bits=self.rng.integers(0, 2, w.bt.ids).astype(np.uint8)) if w.bound_ok() else None

    def d_pdb_load(self, hint):
        w, rng = self.w, self.rng
        if not w.bound_ok():
            return None
        n_pdb = int(rng.integers(1, 9))
        off, member = pdr.random_members(rng, w.bt.ids, n_pdb)
        return dict(allowed=pdr.random_allowed(rng, n_pdb), off=off, member=member)

    def d_pdb_append(self, hint):
        w, rng = self.w, self.rng
        if not w.bound_ok() or w.pm is None or w.pm.covered >= w.bt.ids:
            return None
        c = int(rng.integers(1, w.bt.ids - w.pm.covered + 1))
        off, member = pdr.random_members(rng, c, w.pm.n_pdb, sizes=(0, 1, 3))
        return dict(off=off, member=member)

    def d_pdb_allowed(self, hint):
        w, rng = self.w, self.rng
        if not w.bound_ok() or w.pm is None:
            return None
        idx = rng.permutation(w.pm.n_pdb)[: int(rng.integers(1, w.pm.n_pdb + 1))].astype(np.uint32)
        return dict(index=idx, value=pdr.random_allowed(rng, idx.size, 0.4))

    # -- preemption
    def _preemptors(self, gang):
        w, rng = self.w, self.rng
        if w.preempt_ok() != OK or not w.pods.p:
            return None
        pool = w.unplaced if w.unplaced is not None and w.unplaced.size else np.nonzero(w.pods.group >= 0)[0]
        if not pool.size:
            return None
        idx = np.sort(rng.permutation(pool)[: int(rng.integers(1, 13))])
        grp = w.pods.group[idx]
        prio = np.where(grp >= 0, self.sc["gprio"][np.clip(grp, 0, 63)], 350).astype(np.int32)
        if gang:
            o = capi.gang_order(grp, prio)
            idx, prio = idx[o], prio[o]
        prot = (rng.random(w.g) < 0.1).astype(np.uint8)
        return dict(pod_index=idx.astype(np.uint32), priority=prio, protected=prot)

    def d_preempt(self, hint):
        return self._preemptors(False)

    def d_commit(self, hint):
        if hint == "clear_same":           # the preemptors of the last plan-only commit, now applied with BS_PREEMPT_CLEAR_LOWER
            if self.planned is None or self.w.preempt_ok() != OK or int(self.planned["pod_index"].max()) >= self.w.pods.p:
                return None
            a, self.planned = dict(self.planned, apply=True, clear_lower=True), None
            return a
        a = self._preemptors(False)
        if a is None:
            return None
        u = self.rng.random()
        apply = hint in ("apply", "assume") or u < 0.6
        assume = hint == "assume" or (hint is None and apply and u < 0.3)
        return self._flags(dict(a, apply=bool(apply), assume=bool(assume)), hint)

    def d_commit_gang(self, hint):
        w, rng = self.w, self.rng
        a = self._preemptors(True)
        if a is None:
            return None
        grp = w.pods.group[a["pod_index"]]
        need = np.zeros(w.g, np.uint32)
        for x in np.unique(grp[grp >= 0]):
            c = int((grp == x).sum())
            need[x] = rng.choice([0, 1, c, c + 1])                              # no requirement, an easy one, everybody, one more than there are
        u = rng.random()
        apply = hint == "apply" or u < 0.6
        if hint == "nominate_void" and np.any(grp >= 0):                        # the first gang asks for one more than it sends: its run is voided
            x = int(grp[grp >= 0][0])
            need[x] = int((grp == x).sum()) + 1
        return self._flags(dict(a, need=need, apply=bool(apply), assume=bool(apply and u < 0.3)), hint)

    # -- the nominated-pod table and the two passes that came with it (plan_nom only: plan draws none of these)
    def _prio(self, idx):
        """the priority of queue pods: the scene's, by group (a pod without a group: 350), as _preemptors gives it"""
        grp = self.w.pods.group[idx]
        return np.where(grp >= 0, self.sc["gprio"][np.clip(grp, 0, 63)], 350).astype(np.int32)

    def _flags(self, a, hint):
        """the two flags on a drawn commit: by hint, else (plan_nom only) at random where they are legal"""
        w, rng = self.w, self.rng
        if not self.nom:
            return a
        if hint == "plan":                 # the plan only, for preemptors above every row: where they stand does not depend on rows below them
            a.update(priority=np.full(len(a["pod_index"]), 6000, np.int32), apply=False, assume=False, nominate=False, clear_lower=False)
            self.planned = dict(a)
            return a
        if hint in ("nominate", "nom_clear", "clear", "nominate_void", "nominate_top"):
            if hint != "clear" and not w.nom_ok():
                return None
            a.update(apply=True, assume=False if hint != "clear" else bool(a["assume"]), nominate=hint != "clear",
                     clear_lower=hint in ("nom_clear", "clear") or bool(rng.random() < 0.4 and hint != "nominate_top"))
            if hint in ("clear", "nominate_top"):      # preemptors above every row: no row turns them away; whatever node they stand on, "clear" clears its rows
                a["priority"] = np.full(len(a["pod_index"]), 6000, np.int32)
            return a
        u = rng.random()
        nominate = bool(w.nom_ok() and a["apply"] and not a["assume"] and u < 0.6)
        a.update(nominate=nominate, clear_lower=bool(rng.random() < 0.5))
        return a

    def d_nom_load(self, hint):
        """"empty": the empty table; "grow": rows of which one FREES room (a negative cpu lane: the fit test of its node sees more than the
        node has); else up to 30 rows with queue pods' requests, half of them asking for half of what their node has left"""
        w, rng = self.w, self.rng
        L = 4 + w.S
        if hint == "empty" or not w.pods.p:
            return dict(node=np.zeros(0, np.uint32), priority=np.zeros(0, np.int32), req=np.zeros((L, 0), np.int64), req_present=np.zeros(0, np.uint32))
        m = 204 if hint == "big" else int(rng.integers(4, 31))                   # (204 rows: the largest table laid out for the smallest allocation, 256 rows)
        node = rng.integers(0, w.n, m).astype(np.uint32)
        src = rng.integers(0, w.pods.p, m)
        prio = (self._prio(src).astype(np.int64) + rng.integers(-1, 2, m)).astype(np.int32)
        req = w.pods.req[:L, src].astype(np.int64).copy()
        free = np.maximum(w.nl.alloc[0] - w.nl.req[0], 0)[node]
        req[0] = np.where(rng.random(m) < 0.5, free // 2 + req[0], req[0])
        if hint == "grow":
            full = np.nonzero(w.nl.alloc[0] - w.nl.req[0] < 20)[0]             # a node too full for most pods: the row makes room on it for the test
            node[0] = int(rng.choice(full)) if full.size else node[0]
            req[0, 0], prio[0] = -int(rng.integers(50, 400)), 6000
        return dict(node=node, priority=prio, req=req, req_present=w.pods.req_present[src].copy())

    def d_nom_apply(self, hint):
        """"created": removes an id the last preemption call created; "grow": removes the rows with a negative lane; else up to three live
        ids leave and up to four queue pods without a row enter on random nodes"""
        w, rng = self.w, self.rng
        if not w.nom_ok():
            return None
        live = w.nt.id
        if hint == "created":
            made = w.pre_nom[np.isin(w.pre_nom, live)] if w.pre_nom is not None else np.zeros(0, np.uint32)
            if not made.size:
                return None
            remove = rng.permutation(made)[:1]
        elif hint == "grow":
            remove = live[np.any(w.nt.req < 0, axis=0)]
            if not remove.size:
                return None
        else:
            remove = rng.permutation(live)[: int(rng.integers(0, min(live.size, 3) + 1))]
        free = np.nonzero(w.own == NOM_NONE)[0]
        idx = np.sort(rng.permutation(free)[: int(rng.integers(0 if remove.size else 1, 5))]) if hint is None else np.zeros(0, np.int64)
        if hint == "under":                # a row of a queue pod on every node the last (plan-only) commit stands on
            res = self.last_out.get("res") if self.last_out else None
            nodes = np.unique(res["node"][res["node"] >= 0]) if res is not None else np.zeros(0, np.int64)
            free = free[np.isin(free, self.planned["pod_index"], invert=True)] if self.planned is not None else free
            k = min(nodes.size, free.size)
            if not k:
                return None
            idx = free[:k]
            return dict(remove=np.zeros(0, np.uint32), pod_index=idx.astype(np.uint32), node=nodes[:k].astype(np.uint32), priority=self._prio(idx))
        if hint == "many":                 # up to 256 rows: the next row takes the table past the smallest allocation
            k = 256 - int(live.size)
            if k <= 0 or not w.pods.p:
                return None
            remove, idx = np.zeros(0, np.uint32), np.sort(rng.choice(w.pods.p, k, replace=k > w.pods.p))
        if not remove.size and not idx.size:
            return None
        return dict(remove=np.asarray(remove, np.uint32), pod_index=idx.astype(np.uint32), node=rng.integers(0, w.n, idx.size).astype(np.uint32), priority=self._prio(idx))

    def d_nom_nodes(self, hint):
        return dict() if self.w.nt is not None and self.w.pend_n else None

    def d_pass_nom(self, hint):
        w = self.w
        if not w.nom_ok() or not w.pods.p:
            return None
        if hint == "rows" and not w.nt.id.size:
            return None
        return dict(priority=self._prio(np.arange(w.pods.p)), own_id=w.own.copy())

    def d_pass_scored(self, hint):
        if not self.w.pods.p:
            return None
        ws = sss.WEIGHTS + [(0, 1, 0)]
        return dict(weights=ws[int(self.rng.integers(0, len(ws)))])

    # -- calls the header refuses
    def d_refuse(self, hint):
        """-> (kind, args) of a call the model predicts a refusal for, or None"""
        w, rng = self.w, self.rng
        self.owed = None
        if hint in NOM_REFUSALS:
            return self._refuse_nom(hint)
        if hint == "stale_wait":
            if w.wt is None or w.wt.n == w.n:
                return None
            if w.wt.w and rng.random() < 0.7:
                gs = [int(w.wt.group[0])]
                return ("expire", dict(groups=gs, deny=True)) if rng.random() < 0.5 else ("release", dict(groups=gs))
            return ("forget", dict(ids=w.wt.id[:1].astype(np.uint32))) if w.wt.w else ("park", dict())
        if hint == "stale_bound":
            if w.bt is None or w.bt.n == w.n:
                return None
            u = rng.random()
            if u < 0.4:
                return "bound_apply_ex", dict(remove=w.bt.id[:1].astype(np.uint32), insert=None, pdb=None)
            pi = np.zeros(1, np.uint32)
            if u < 0.7:
                return "preempt", dict(pod_index=pi, priority=np.full(1, 350, np.int32), protected=np.zeros(w.g, np.uint8))
            return "commit", dict(pod_index=pi, priority=np.full(1, 350, np.int32), protected=np.zeros(w.g, np.uint8), apply=True, assume=False)
        if hint == "window":
            if w.window or w.pend_w:
                return None
            if w.wait_ok() and rng.random() < 0.5:
                return "park", dict()
            return "seq_expire", dict(groups=[0], deny=False, all=False)
        if hint == "list_order":
            a, b = sorted(rng.choice(w.g, 2, replace=False).tolist())
            return "list", dict(remove=[b, a] if rng.random() < 0.5 else [a, a], update=[], rows=new_group_rows(rng, w.S, 0), n_append=0)
        if hint == "forget_dead":
            if not w.wait_ok() or w.wt.w < 2 or w.pend_w or w.pend_b:
                return None
            dead = np.setdiff1d(np.arange(w.wt.ids), w.wt.id)
            bad = int(rng.choice(dead)) if dead.size else w.wt.ids
            return "forget", dict(ids=np.array([int(w.wt.id[0]), bad], np.uint32))
        if hint == "expire_twice":
            if not w.wait_ok() or w.wt.w < 2 or w.pend_w or w.pend_b:
                return None
            x = int(w.wt.group[0])
            return "expire", dict(groups=[x, x], deny=True)
        if hint == "bind_stale":           # between node-list surgery and the *_nodes_apply calls; with only pods listed too (surgery shut the window)
            if w.bt is None or (w.bt.n == w.n and (w.wt is None or w.wt.n == w.n)):
                return None
            live = w.wt is not None and w.wt.w and (w.bt.n == w.n or rng.random() < 0.5)
            if not live and not w.pods.p:
                return None
            return "bind", self._bind_args(w.wt.id[:1], []) if live else self._bind_args([], [int(rng.integers(0, w.pods.p))])
        if hint == "bind_window":
            if w.window or not w.bound_ok() or w.pend_w or w.pend_b or not w.pods.p:
                return None
            return "bind", self._bind_args([], [int(rng.integers(0, w.pods.p))])
        if hint in ("bind_waits", "bind_dead"):
            if not w.bound_ok() or not w.wait_ok() or not w.wt.w or not w.window or w.pend_w or w.pend_b:
                return None
            live = int(rng.choice(w.wt.id))
            free = self._bindable()
            if hint == "bind_waits":       # a pod the pass left waiting that nobody has parked or expired: the kernels find it, after the marks were set
                waits = np.nonzero(w.wait_node >= 0)[0]
                if not waits.size:
                    return None
                got = "bind", self._bind_args([live], [int(p) for p in free[:1]] + [int(rng.choice(waits))])
            else:                          # a dead id beside a live one and a pod that would bind
                dead = np.setdiff1d(np.arange(w.wt.ids), w.wt.id)
                if not dead.size or not free.size:
                    return None
                got = "bind", self._bind_args([live, int(rng.choice(dead))], [int(rng.choice(free))])
            self.owed = ("forget", dict(ids=np.array([live], np.uint32)))
            return got
        raise KeyError(hint)

    def _refuse_nom(self, hint):
        """the refusals of the nominated-pod table's calls (Drawer.d_refuse): each has ONE cause, all are found on the host"""
        w, rng = self.w, self.rng
        one = dict(pod_index=np.zeros(1, np.uint32), priority=np.full(1, 350, np.int32), protected=np.zeros(w.g, np.uint8))
        if hint == "nom_before_load":
            if w.nt is not None:
                return None
            if w.pods.p and rng.random() < 0.5:
                return "pass_nom", dict(priority=self._prio(np.arange(w.pods.p)), own_id=None)
            return "nom_apply", dict(remove=np.zeros(0, np.uint32), pod_index=np.zeros(1, np.uint32), node=np.zeros(1, np.uint32), priority=np.zeros(1, np.int32))
        if w.nt is None or not w.pods.p:
            return None
        prio = self._prio(np.arange(w.pods.p))
        def preemption(why):
            """the three preemption calls in turn, per cause (the stale bound table; the nominated-pod table alone)"""
            t = self.turn[why] = self.turn[why] + 1
            t = (t + int(self.sc.get("seed", 0))) % 3
            if t == 0:
                return "preempt", one
            if t == 1:
                return "commit", dict(one, apply=True, assume=False, nominate=False, clear_lower=True)
            return "commit_gang", dict(one, need=np.zeros(w.g, np.uint32), apply=False, assume=False, nominate=False, clear_lower=False)

        nom_rows_stale = w.nt.n != w.n and w.nt.id.size > 0 and w.bound_ok()      # the nominated-pod table alone makes a preemption call refuse
        if hint == "stale_between":        # between two *_nodes_apply: what the tables that have not followed yet refuse
            hint = "stale_preempt" if nom_rows_stale or w.nt.n == w.n else "stale_nom"
        if hint == "stale_preempt":        # a preemption call while the bound table, or the nominated-pod table with rows, has not followed
            if w.bt is None or (w.bound_ok() and not nom_rows_stale):
                return None
            return preemption("stale_nom" if nom_rows_stale else "stale_bound")
        if hint == "stale_nom":
            if w.nt.n == w.n:
                return None
            u = rng.random()
            if nom_rows_stale and u < 0.4:
                return preemption("stale_nom")
            self.turn["stale_call"] = self.turn.get("stale_call", 0) + 1
            if (self.turn["stale_call"] + int(self.sc.get("seed", 0))) % 2 or not w.nt.id.size:                      # the two nominated calls in turn
                return "pass_nom", dict(priority=prio, own_id=w.own.copy())
            return "nom_apply", dict(remove=w.nt.id[:1].copy(), pod_index=np.zeros(0, np.uint32), node=np.zeros(0, np.uint32), priority=np.zeros(0, np.int32))
        if not w.nom_ok():
            return None
        dead = np.setdiff1d(np.arange(w.nt.ids, dtype=np.uint32), w.nt.id)
        if hint == "pass_nom_filter":
            return "pass_nom", dict(priority=prio, own_id=w.own.copy(), filter=True)
        if hint in ("own_dead", "own_dropped", "own_cleared"):
            # dead: consumed by a pass, dropped with its node, cleared by a commit, removed by bs_nominated_apply; or past the id space.  The
            # cause this drawer has used least, among those the table's history offers ("own_dropped", "own_cleared": that cause or nothing)
            by = {c: [i for i, why in w.died.items() if why == c] for c in DEATHS[:-1]}
            by["unknown"] = [int(w.nt.ids)]
            assert sorted(x for c in DEATHS[:-1] for x in by[c]) == dead.tolist(), "every dead id has its cause"
            want = {"own_dropped": ["dropped"], "own_cleared": ["cleared"]}.get(hint, list(DEATHS))
            prefer = ("consumed", "removed", "unknown", "dropped", "cleared")        # (the last two have hints, and motifs, of their own)
            have = sorted((c for c in want if by[c]), key=lambda c: (self.death_used[c], prefer.index(c)))
            if not have:
                return None
            self.death_used[have[0]] += 1
            own = w.own.copy()
            own[int(rng.integers(0, w.pods.p))] = int(rng.choice(by[have[0]]))
            return "pass_nom", dict(priority=prio, own_id=own)
        if hint == "own_twice":
            if not w.nt.id.size or w.pods.p < 2:
                return None
            own = w.own.copy()
            a, b = rng.choice(w.pods.p, 2, replace=False)
            own[a] = own[b] = int(rng.choice(w.nt.id))
            return "pass_nom", dict(priority=prio, own_id=own)
        if hint == "nom_remove_dead":
            if not dead.size:
                return None
            rm = np.concatenate([w.nt.id[:1], rng.permutation(dead)[:1]]).astype(np.uint32)
            return "nom_apply", dict(remove=rm, pod_index=np.zeros(0, np.uint32), node=np.zeros(0, np.uint32), priority=np.zeros(0, np.int32))
        raise KeyError(hint)


NOM_REFUSALS = ["stale_nom", "stale_preempt", "stale_between", "own_dead", "own_dropped", "own_cleared", "own_twice", "nom_remove_dead", "nom_before_load", "pass_nom_filter"]


def plan(seed: int, orc):
    """-> (scene, steps): steps = [(kind, args, refused)] drawn on a World of the plan's own.  The first two calls load the (empty) wait
    table and the bound table.  Then four motifs per seed (two of MOTIF_ORDER, two of MOTIF_ORDER_BIND, in rotation over the seeds), with
    single calls between them: the single call is of the row of calls (ROWS) this seed has used least so far, and within the row the entry
    point used least.  Every sixth step is a call the model predicts a refusal for.  A call that is not applicable is drawn again as
    another call, never skipped; the four refusals the device finds (ON_DEVICE) are each followed by a successful call of the same
    removal core: a refused bind by the forget of the live id it listed."""
    sc = scene(seed)
    w = world_of(orc, sc)
    rng = np.random.default_rng(88000 + seed)
    dr = Drawer(w, sc, rng)
    steps, queue = [], []
    used = dict.fromkeys(ROW_OF, 0)
    want = 2 if seed % 4 == 0 else 3       # calls of every row: 2 in every seed, 30 over the twelve

    def do(kind, args, refused=False):
        out = w.step(kind, args)
        assert (out["status"] != OK) == refused, f"seed {seed} step {len(steps)} {kind}: status {out['status']} drawn as {'a refusal' if refused else 'a call'}"
        if not refused:
            used[kind] += 1
        steps.append((kind, args, refused))

    def single():
        """the least used row's least used entry point that is applicable now"""
        row_used = {r: sum(used[k] for k in ROWS[r]) for r in ROWS}
        if len(steps) > 12 and rng.random() < 0.06:                              # a table loaded afresh in mid-sequence: its ids restart
            k = "wait_load" if used["wait_load"] <= used["bound_load"] else "bound_load"
            a = dr.draw(k)
            if a is not None:
                return [(k, a)]
        score = lambda k: (min(row_used[ROW_OF[k]], want), used[k] > 0, row_used[ROW_OF[k]] + used[k], rng.random())   # a row `want` times, then an entry point once
        for k in sorted(ROW_OF, key=score):
            a = dr.draw(k)
            if a is not None:
                return [(k, a)]
            if k == "seq_expire" and not w.window and dr.draw("pass") is not None:
                return ["pass", "seq_expire"]                                   # the window is shut or nobody waits: a pass opens it
        raise AssertionError(f"seed {seed}: no call is applicable at step {len(steps)}")

    def room_for(motif):
        """the steps left hold the motif, the refusals due, and what the rows lack of `want` calls each once the motif has run"""
        after = {r: sum(used[k] for k in ROWS[r]) for r in ROWS}
        for item in motif:
            k = item if isinstance(item, str) else item[0]
            if k in ROW_OF:
                after[ROW_OF[k]] += 1
        left = STEPS - len(steps)
        return left >= len(motif) + left // 6 + 1 + sum(max(0, want - c) for c in after.values())

    do("wait_load", dict(node=(), group=(), req=None, req_present=None))
    do("bound_load", dict(bound=sc["bound"]))
    motifs = [MOTIF_ORDER[seed % 4], MOTIF_ORDER_BIND[seed % 3], MOTIF_ORDER[(seed + 2) % 4], MOTIF_ORDER_BIND[(seed + 1) % 3]]
    on_device = set(ON_DEVICE)                                                   # each once per seed: they cost a second call
    if sc["nodes"].n <= 5 and "c" not in motifs:
        motifs[0] = "c"                    # this seed takes its node count down across 4
    if sc["nodes"].n > 60 and "e" not in motifs:
        motifs[0] = "e"                    # and this one up across 64
    after = None                           # a successful call owed after a refusal the device found
    gap = 0
    # the first cycle: its pass leaves gangs waiting that share nodes.  (Seed 0 binds in the new form too: its bound table is the empty one)
    queue, opening = list(OPENING_BIND if seed % 2 or not sc["bound"].b else OPENING), True
    while len(steps) < STEPS:
        if after is not None:
            kind, after = after, None
            a = dr.draw(kind) if isinstance(kind, str) else kind[1]
            kind = kind if isinstance(kind, str) else kind[0]
            assert a is not None, f"seed {seed}: the {kind} owed after a refusal on the device is not applicable"
            do(kind, a)
            continue
        if len(steps) % 6 == 5 and 6 * sum(r for _, _, r in steps) < len(steps) + 1:       # a sixth, the motifs' own refusals included
            order = list(rng.permutation(REFUSALS))
            if w.pend_w or w.pend_b:
                order = [str(x) for x in rng.permutation(["stale_wait", "stale_bound", "bind_stale"])] + order
            for r in order:
                got = dr.d_refuse(r) if r not in ON_DEVICE or r in on_device else None
                if got is not None:
                    do(got[0], got[1], refused=True)
                    after = dr.owed or {"forget_dead": "forget", "expire_twice": "expire"}.get(r)
                    on_device.discard(r)
                    break
            else:
                raise AssertionError(f"seed {seed}: no refusal is applicable at step {len(steps)}")
            continue
        if not queue:
            opening = False
            if w.pend_w or w.pend_b:       # node-list surgery is followed first, in either order
                queue = [str(k) for k in rng.permutation(["wait_nodes", "bound_nodes"])]
            elif motifs and gap >= 1 and room_for(MOTIFS[motifs[0]]):
                DEBUG and print(f"seed {seed} step {len(steps)}: motif {motifs[0]}")
                queue, gap = list(MOTIFS[motifs.pop(0)]), 0                     # (there is room for it and for what the rows still lack)
            else:
                queue, gap = single(), gap + 1
        item = queue.pop(0)
        if isinstance(item, tuple) and isinstance(item[1], dict):
            do(*item)
            continue
        kind, hint = (item, None) if isinstance(item, str) else item
        if kind == "refuse":
            got = dr.d_refuse(hint) if hint not in ON_DEVICE or hint in on_device else None
            if got is not None:
                do(got[0], got[1], refused=True)
                after = dr.owed
                on_device.discard(hint)
            continue
        a = dr.draw(kind, hint)
        if a is None:                      # not applicable: the rest of the motif goes with it, other calls are drawn
            DEBUG and print(f"seed {seed} step {len(steps)}: {item} is not applicable, dropped with {queue}")
            queue = queue if opening else []
            continue
        do(kind, a)
    return sc, steps


# ======================================================================================================================================
# the second plan family: the nominated-pod table, BS_PREEMPT_NOMINATE / _CLEAR_LOWER, bs_seq_run_nominated and bs_seq_run_scored
# ======================================================================================================================================
NOM_SEEDS = 8                               # scene(seed): S in 0, 1, 2, 12 twice; seed 0 crosses 4 nodes downwards, seed 1 crosses 64 upwards with rows
NODES_APPLY = ("nom_nodes", "wait_nodes", "bound_nodes")
NODES_ORDERS = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
# the hazards of tests/test_world_nom_cpu.py as call sequences
NOM_MOTIFS = {
    # (n_a is the opening's own sequence, and n_b's with the preemption call at its end)
    "n_b": [("commit_gang", "nominate"), ("pods", "nominees"), ("pass_nom", "rows"), ("seq_expire", "consumed"), "park_or_bind", "preempt"],
    "n_c": [("commit", "nominate"), ("nodes", "rows"), "follow_refused"],
    "n_d": [("commit", "nominate"), ("nodes", "rows_swap"), "follow"],
    "n_e": [("commit_gang", "nominate_void"), ("nom_apply", "created")],
    "n_f": [("commit", "plan"), ("nom_apply", "under"), ("commit", "clear_same"), ("refuse", "own_cleared"), ("pass_nom", None)],
    "n_g": [("pods", "nominees"), ("assume", "free"), "pass_scored", "pass", ("pass_nom", None), ("pods", "nominees"), ("assume", "free"), "pass_scored"],
    "n_h": [("pods", "nominees"), ("assume", "free"), "pass_scored", ("pods", "resize"), "pass"],
    "n_i": [("commit", "nominate"), ("list", "resize"), ("pass_nom", "rows")],
    "n_j": [("nom_load", "big"), ("nom_apply", "many"), ("commit_gang", "nominate_top"), ("nodes", "grow"), ("refuse", "stale_nom"), "nom_nodes", "follow", ("nom_load", None)],
    # (not a hazard of its own: the bound table follows first, so the nominated-pod table ALONE refuses the preemption calls; then a pass names
    # an id that died with its node)
    "n_l": [("nom_load", None), ("commit", "nominate"), ("nodes", "rows"), ("refuse", "stale_nom"), "bound_nodes", ("refuse", "stale_preempt"), "wait_nodes",
            "nom_nodes", ("refuse", "own_dropped"), ("pods", "nominees"), ("pass_nom", "rows")],
    "n_k": [("nom_load", "grow"), ("pass_nom", "rows"), ("pods", "nominees"), ("nom_apply", "grow"), ("pass_nom", None)],
}
NOM_MOTIF_ORDER = [m for m in NOM_MOTIFS if m not in ("n_b", "n_f", "n_l")]     # (n_f and n_l lead every seed; n_b's tail follows any pass that allows it)
NOM_OPENING = [("pass", None), ("commit_gang", "nominate"), ("bind", "cycle"), ("park", None), ("pods", "nominees"), ("pass_nom", None), ("commit", "nom_clear")]
PERIODIC = ["own_dead", "own_twice", "own_dead", "nom_remove_dead", "host", "own_dead", "pass_nom_filter", "host"]
HOST_REFUSALS = ["stale_wait", "stale_bound", "window", "list_order", "bind_stale", "bind_window"]     # the first family's that need no second call


def plan_nom(seed: int, orc):
    """-> (scene, steps) as plan(): STEPS steps on scene(seed).  The opening is the header's cycle with nomination (the three tables loaded,
    the nominated one empty; pass; a gang commit that nominates; bind and park; the queue moves on with the nominees in it; a pass under rule
    S with their own ids; a commit that nominates and clears).  Then n_f and n_l in every seed (rows are cleared; the bound table follows
    surgery first, so that the nominated-pod table alone refuses a preemption call, and a pass names an id that died with its node), then
    the other motifs of NOM_MOTIFS in rotation, with single calls once they are used up: the entry point of NOM_ROW_OF this seed has used
    least.  After any pass under rule S outside the opening whose consumed pod still waits, that gang times out in the same window (n_b's
    tail, twice per seed at most).  Node-list surgery is followed by the three *_nodes_apply in one of their six orders, in rotation.  Every
    sixth step is a call the model predicts a refusal for, the motifs' own included; the others go through PERIODIC in turn, and the drawer
    takes the three preemption calls, the two nominated calls and the causes of a dead own id in turn as well."""
    sc = scene(seed)
    w = world_of(orc, sc)
    rng = np.random.default_rng(89000 + seed)
    dr = Drawer(w, sc, rng)
    dr.nom = True
    steps, used, order_no, periodic, expired = [], dict.fromkeys(NOM_ROW_OF, 0), [seed], [0], [0]

    def do(kind, args, refused=False):
        out = w.step(kind, args)
        assert (out["status"] != OK) == refused, f"nom seed {seed} step {len(steps)} {kind}: status {out['status']} drawn as {'a refusal' if refused else 'a call'}"
        if not refused:
            used[kind] += 1
            dr.last_out = out
        steps.append((kind, args, refused))

    def refuse(hints):
        for h in hints:
            got = dr.d_refuse(h)
            if got is not None:
                do(got[0], got[1], refused=True)
                return True
        return False

    def follow(refused_between):
        """the *_nodes_apply the tables owe, in the next of the six orders"""
        order = [NODES_APPLY[j] for j in NODES_ORDERS[order_no[0] % 6]]
        order_no[0] += 1
        out = [k for k in order if dr.draw(k) is not None]
        if refused_between and len(out) == 3:
            out = [out[0], ("refuse", "stale_between"), out[1], out[2]]
        return out

    do("wait_load", dict(node=(), group=(), req=None, req_present=None))
    do("bound_load", dict(bound=sc["bound"]))
    refuse(["nom_before_load"])
    do("nom_load", dr.draw("nom_load", "empty"))
    queue, opening = list(NOM_OPENING), True
    motifs = [NOM_MOTIF_ORDER[(5 * seed + j) % len(NOM_MOTIF_ORDER)] for j in range(len(NOM_MOTIF_ORDER))]
    motifs = ["n_f", "n_l"] + motifs                                           # (every seed clears rows, and drops rows with a node)
    if sc["nodes"].n > 60:
        motifs.insert(0, "n_j")             # this seed takes its node count up across 64 with rows in the table
    while len(steps) < STEPS:
        if len(steps) % 6 == 5 and 6 * sum(r for _, _, r in steps) < len(steps) + 1 and not (queue and queue[0] == ("refuse", "stale_between")):
            # the refusals no motif makes, in turn (an own id that is dead every other time: it has five causes, taken in turn themselves)
            stale = [str(x) for x in rng.permutation(["stale_nom", "stale_wait", "stale_bound", "bind_stale"])] if w.pend_w or w.pend_b or w.pend_n else []
            at = (3 * seed + periodic[0]) % len(PERIODIC)
            periodic[0] += 1
            hints = [h for x in PERIODIC[at:] + PERIODIC[:at] for h in ([str(y) for y in rng.permutation(HOST_REFUSALS)] if x == "host" else [x])]
            assert refuse(stale + hints), f"nom seed {seed}: no refusal is applicable at step {len(steps)}"
            continue
        if not queue:
            opening = False
            if w.pend_w or w.pend_b or w.pend_n:
                queue = follow(False)
            elif motifs and STEPS - len(steps) >= len(NOM_MOTIFS[motifs[0]]) + 2:
                DEBUG and print(f"nom seed {seed} step {len(steps)}: motif {motifs[0]}")
                queue = list(NOM_MOTIFS[motifs.pop(0)])
            else:
                for k in sorted(NOM_ROW_OF, key=lambda k: (used[k], rng.random())):
                    a = dr.draw(k)
                    if a is not None:
                        queue = [(k, a)]
                        break
            continue
        item = queue.pop(0)
        if item in ("follow", "follow_refused"):
            queue = follow(item == "follow_refused") + queue
            continue
        kind, hint = (item, None) if isinstance(item, str) else item
        if isinstance(hint, dict):
            do(kind, hint)
            continue
        if kind == "refuse":
            if hint == "stale_between":    # between two *_nodes_apply: a nominated call or a preemption call that a table which has not followed refuses
                refuse(["stale_between"])
            else:
                refuse([hint])
            continue
        if kind == "park_or_bind":         # whichever the window still offers; neither: the next item
            for k, h in (("park", None), ("bind", "pods")):
                a = dr.draw(k, h)
                if a is not None:
                    do(k, a)
                    break
            continue
        a = dr.draw(kind, hint)
        if a is None:
            DEBUG and print(f"nom seed {seed} step {len(steps)}: {item} is not applicable, dropped with {queue}")
            queue = queue if opening else []
            continue
        do(kind, a)
        if kind == "pass_nom" and not opening and expired[0] < 2 and not (queue and queue[0] == ("seq_expire", "consumed")) and dr.draw("seq_expire", "consumed") is not None:
            # a consumed pod still waits at Permit: its gang times out in this window, whichever motif the pass belongs to (hazard n_b)
            expired[0] += 1
            queue = [("seq_expire", "consumed"), "park_or_bind"] + queue
    return sc, steps
