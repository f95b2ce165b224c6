"""GPU tests of bs_seq_expire / bs_seq_waiting_read (csrc/bs_seq_expire.hpp) — a gang's Permit timeout after bs_seq_run — against the
array-level model of tests/seq_expire_ref.py, bit for bit: all of bs_seq_expire_out, bs_nodes_read and bs_groups_read after the call,
bs_find_max_pg against the oracle on the model's group state, and what follows on the context (a batch and a second pass answer as a twin
context that loaded the model's state).  The FILTER-stage passes are held against the object-level statement."""
import numpy as np
import pytest

import naive_ref as nv
import seq_expire_ref as ser
import seq_obj_replay as sor
from test_gpu_parity import load_ctx
from test_gpu_seq import assert_groups_equal
from test_seq_oracle_pin import _with_waiting

pytestmark = pytest.mark.gpu
I64MIN, I64MAX = -(1 << 63), (1 << 63) - 1


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def waiting_scene(soa, lens, n_nodes=8, S=0, pods_cap=110, interleave=False, matched0=None, closed=(), skip_nodes=0, seed=0):
    """gang g has lens[g] pods in the queue and MinMember lens[g] + matched0[g] + 1: nobody reaches the quorum, every pod that finds a node
    waits.  Roomy nodes, first fit fills node 0's pods lane (pods_cap) and moves on.  closed: groups in a phase that releases nobody
    (MinMember 1: their pods are ready at once and still wait).  skip_nodes: the first nodes are unschedulable.  S scalar lanes: every
    node has the allocatable keys, every second node lacks the requested keys (the assume step creates them)."""
    rng = np.random.default_rng(seed)
    G, L, N = len(lens), 4 + S, n_nodes
    matched0 = [0] * G if matched0 is None else matched0
    alloc = np.zeros((L, N), np.int64)
    alloc[0], alloc[1], alloc[2], alloc[3] = 10 ** 7, 1 << 44, 1 << 44, pods_cap
    alloc[4:] = 10 ** 6
    reqd = np.zeros((L, N), np.int64)
    reqd[0] = rng.integers(0, 1000, N)
    reqd[1] = rng.integers(0, 1 << 30, N)
    reqd[4:] = rng.integers(0, 50, (S, N))
    ap = np.full(N, (1 << S) - 1, np.uint32)
    rp = np.where(np.arange(N) % 2 == 0, (1 << S) - 1, 0).astype(np.uint32)
    flags = np.zeros(N, np.uint8)
    flags[:skip_nodes] = soa.NODE_UNSCHEDULABLE
    nodes = soa.Nodes(alloc, reqd, ap, rp, flags)
    fit = soa.FitMasks.from_bool(np.ones((1, N), bool))
    groups = soa.Groups.empty(G, L)
    groups.min_member[:] = [1 if g in closed else lens[g] + matched0[g] + 1 for g in range(G)]
    groups.matched[:] = matched0
    for g in closed:
        groups.flags[g] |= soa.GROUP_PHASE_CLOSED
    if interleave:
        left, order = list(lens), []
        while any(left):
            for g in range(G):
                if left[g]:
                    order.append(g)
                    left[g] -= 1
        group = np.array(order, np.int32)
    else:
        group = np.repeat(np.arange(G, dtype=np.int32), lens)
    P = group.size
    req = np.zeros((L, P), np.int64)
    req[0] = rng.integers(1, 20, P)
    req[1] = rng.integers(1, 1 << 20, P)
    pres = (rng.integers(0, 1 << S, P) if S else np.zeros(P, np.int64)).astype(np.uint32)
    req[4:] = rng.integers(1, 4, (S, P)) * ((pres[None, :] >> np.arange(S, dtype=np.uint32)[:, None]) & 1)
    pods = soa.Pods(group, req, pres, np.zeros(P, np.uint32), np.zeros(P, np.uint64), np.zeros(P, np.uint8))
    return nodes, fit, groups, pods


# ---- the harness -------------------------------------------------------------------------------------------------------------------------
class Case:
    """a context that ran one PREFILTER pass over the scene, and the array model of the same state"""

    def __init__(self, bsa, soa, orc, scene, check_pass=True):
        self.bsa, self.soa, self.orc = bsa, soa, orc
        self.nodes, self.fit, self.groups, self.pods = scene
        self.s = orc.seq_replay(self.nodes, self.fit, self.groups, self.pods, soa.STAGE_PREFILTER)
        self.st = ser.State.after_pass(self.nodes, self.fit, self.groups, self.pods, self.s)     # (asserts that the replay reproduces the oracle)
        self.mg = self.s["groups"].copy()
        self.ctx = load_ctx(bsa, self.nodes, self.fit, self.groups, self.pods)
        r = self.ctx.seq_run(soa.STAGE_PREFILTER)
        if check_pass:
            assert np.array_equal(r["pod_node"], self.s["pod_node"]) and np.array_equal(r["pf_code"], self.s["pf_code"])
        self.check_state("after the pass")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()

    def model_groups(self):
        self.mg.matched[:] = self.st.matched
        self.mg.flags[:] = self.st.flags
        return self.mg

    def model_nodes(self):
        return self.soa.Nodes(self.nodes.allocatable, self.st.requested, self.nodes.allocatable_present, self.st.requested_present, self.nodes.flags)

    def check_state(self, where):
        req, pres = self.ctx.read_node_requests()
        assert np.array_equal(pres, self.st.requested_present), f"{where}: node request keys"
        bad = np.nonzero(req != self.st.requested)
        assert bad[0].size == 0, f"{where}: node requests differ first at lane {bad[0][0]} node {bad[1][0]}: {req[bad][0]} vs {self.st.requested[bad][0]}"
        mg = self.model_groups()
        assert_groups_equal(self.ctx.read_groups(), mg, self.soa, where)
        leader, _, panic = self.orc.find_max_pg(mg)
        assert self.ctx.find_max_pg() == (leader, panic), f"{where}: findMaxPG"
        assert np.array_equal(self.ctx.seq_waiting_read(), self.st.wait_node), f"{where}: bs_seq_waiting_read"

    def expire(self, where, groups=None, deny=False, all=False, group_cap=None, pod_cap=None, flat=False):
        exp = ser.expire(self.st, self.pods, groups=groups, deny=deny, all=all)
        res = self.ctx.seq_expire(groups=groups, deny=deny, all=all, group_cap=group_cap, pod_cap=pod_cap, flat=flat)
        assert (res["n_groups"], res["n_pods"]) == (exp["n_groups"], exp["n_pods"]), f"{where}: counts {res['n_groups']}, {res['n_pods']}"
        kg = exp["n_groups"] if group_cap is None else min(exp["n_groups"], group_cap)
        kp = exp["n_pods"] if pod_cap is None else min(exp["n_pods"], pod_cap)
        for k in ("group", "group_pods", "group_earlier"):
            assert np.array_equal(res[k], exp[k][:kg]), f"{where}: {k}"
        for k in ("pod", "node"):
            assert np.array_equal(res[k], exp[k][:kp]), f"{where}: {k}"
        self.check_state(where)
        return exp

    def follow_up(self, where):
        """a batch and a second pass on the context == on a twin that ran the same first pass (so it carries the same sop.maxFinishedPG)
        and then LOADED the model's node and group state"""
        soa = self.soa
        with load_ctx(self.bsa, self.nodes, self.fit, self.groups, self.pods) as twin:
            twin.seq_run(soa.STAGE_PREFILTER)
            twin.load_nodes(self.model_nodes(), self.fit)
            twin.load_groups(self.model_groups())
            twin.load_pods(self.pods)
            a, b = self.ctx.batch(soa.STAGE_ALL, bitmap=False), twin.batch(soa.STAGE_ALL, bitmap=False)
            for name in ("pf_code", "pf_first_k", "pf_leader", "fl_code", "fl_feasible", "group_admit", "group_ready"):
                assert np.array_equal(getattr(a, name), getattr(b, name)), f"{where}: batch after the expire: {name}"
            ra, rb = self.ctx.seq_run(soa.STAGE_PREFILTER), twin.seq_run(soa.STAGE_PREFILTER)
            for name in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods", "n_released"):
                assert np.array_equal(ra[name], rb[name]), f"{where}: second pass: {name}"
            (qa, pa), (qb, pb) = self.ctx.read_node_requests(), twin.read_node_requests()
            assert np.array_equal(qa, qb) and np.array_equal(pa, pb), f"{where}: node requests after the second pass"
            assert_groups_equal(self.ctx.read_groups(), twin.read_groups(), soa, f"{where}: groups after the second pass")
            assert np.array_equal(self.ctx.seq_waiting_read(), twin.seq_waiting_read()), f"{where}: waiting state after the second pass"


def status_of(bsa, fn):
    with pytest.raises(bsa.BsError) as e:
        fn()
    return e.value.status


# ---- chain and list shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 2, 63, 64, 65, 513])
def test_chain_lengths(length, bsa, soa, orc):
    """513 is one past kSeqWaitList: the pass's LDS list has overflowed and only the global chain holds the gang"""
    with Case(bsa, soa, orc, waiting_scene(soa, [3, length, 2], n_nodes=7, interleave=length < 100, seed=length)) as c:
        assert int((c.pods.group[c.st.wait_node >= 0] == 1).sum()) == length == int(c.st.matched[1])
        others = int((c.st.wait_node >= 0).sum()) - length
        assert others >= 3
        c.expire(f"chain {length}", groups=[1], deny=True)
        assert int((c.st.wait_node >= 0).sum()) == others
        c.follow_up(f"chain {length}")


@pytest.fixture(scope="module")
def many_groups(soa):
    """1100 gangs: every second one has a waiting pod (two for every eighth)"""
    lens = [(2 if g % 8 == 1 else 1) if g % 2 else 0 for g in range(1100)]
    return waiting_scene(soa, lens, n_nodes=9, pods_cap=110, seed=7)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 1025])
def test_listed_group_counts(count, many_groups, bsa, soa, orc):
    """1025 listed groups: one past the scan block (kSeBlock = 1024), the second block's offsets come from the first block's total"""
    rng = np.random.default_rng(count)
    with Case(bsa, soa, orc, many_groups) as c:
        lst = rng.permutation(1100)[:count]
        assert count < 2 or (np.any(lst % 2 == 0) and np.any(lst % 2 == 1))
        if count == 1:
            lst = np.array([1])
        e = c.expire(f"{count} groups", groups=lst, deny=bool(count % 2))
        assert e["n_pods"] >= 1
        c.expire(f"{count} groups, flat form", groups=rng.permutation(1100)[:count], flat=True)
        c.follow_up(f"{count} groups")


def test_all_mode_every_second_group_waiting(many_groups, bsa, soa, orc):
    with Case(bsa, soa, orc, many_groups) as c:
        e = c.expire("ALL", all=True, deny=True)
        assert e["group"].tolist() == list(range(1, 1100, 2)) and e["n_pods"] == int(sum(2 if g % 8 == 1 else 1 for g in range(1, 1100, 2)))
        assert not np.any(c.st.wait_node >= 0)
        e = c.expire("ALL again", all=True)
        assert e["n_groups"] == 0 and e["n_pods"] == 0
        c.follow_up("ALL")


def test_empty_chain_and_a_group_expired_twice(bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [0, 4, 3], n_nodes=3, matched0=[0, 2, 0], seed=3)) as c:
        assert int(c.st.matched[0]) == 0 and not np.any(c.pods.group == 0)
        e = c.expire("empty chain, matched 0", groups=[0])
        assert e["group_pods"].tolist() == [0] and e["group_earlier"].tolist() == [0]
        e = c.expire("first expire", groups=[1, 0])
        assert e["group_pods"].tolist() == [4, 0] and e["group_earlier"].tolist() == [2, 0]
        before = c.st.copy()
        e = c.expire("second expire", groups=[1])
        assert e["n_pods"] == 0 and e["group_earlier"].tolist() == [0]
        assert np.array_equal(before.requested, c.st.requested) and np.array_equal(before.flags, c.st.flags)
        c.follow_up("expired twice")


# ---- node and lane cases -----------------------------------------------------------------------------------------------------------------
def test_64_pods_of_one_gang_on_one_node(bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [64], n_nodes=2, pods_cap=100, seed=4)) as c:
        assert np.all(c.st.wait_node == 0)
        c.expire("64 on one node", groups=[0])
        c.follow_up("64 on one node")


def test_three_gangs_on_one_node(bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [2, 3, 2], n_nodes=1, interleave=True, seed=5)) as c:
        assert np.all(c.st.wait_node == 0) and len(set(c.pods.group.tolist())) == 3
        c.expire("two of three gangs", groups=[2, 0], deny=True)
        c.expire("the third", all=True)
        c.follow_up("three gangs")


@pytest.mark.parametrize("n", [65, 257])
def test_last_node_is_the_one_touched(n, bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [3, 2], n_nodes=n, skip_nodes=n - 1, seed=n)) as c:
        assert np.all(c.st.wait_node == n - 1)
        c.expire("last node", all=True)
        c.follow_up("last node")


@pytest.mark.parametrize("S", [0, 1, 4, 12])
def test_scalar_lane_counts_and_keys_the_assume_created(S, bsa, soa, orc):
    scene = waiting_scene(soa, [5, 4, 6, 3], n_nodes=4, S=S, pods_cap=5, interleave=True, seed=10 + S)
    with Case(bsa, soa, orc, scene) as c:
        nodes, pods = c.nodes, c.pods
        w = c.st.wait_node.copy()
        made = [(i, s) for i in np.nonzero(w >= 0)[0] for s in range(S) if (pods.req_present[i] >> s) & 1 and not (nodes.requested_present[w[i]] >> s) & 1]
        assert S == 0 or made, "a scalar key the assume step created"
        bits0 = c.st.requested_present.copy()
        c.expire(f"S={S}", groups=[2, 0], deny=True)
        c.expire(f"S={S}, the rest", all=True)
        assert np.array_equal(bits0, c.st.requested_present), "the node bits stay"
        for i, s in made:                                      # the word returns to its value: the 0 the assume step started the lane from
            k = w[i]
            if not any(j != i and w[j] == k and (pods.req_present[j] >> s) & 1 for j in range(pods.p) if c.s["pod_node"][j] >= 0):
                assert c.st.requested[4 + s, k] == 0
        c.follow_up(f"S={S}")


def test_int64_extremes_wrap(bsa, soa, orc):
    """node 0 holds INT64_MAX cpu already and the waiting pods ask for negative cpu down to INT64_MIN (a negative request always fits): the
    assume step's sums wrap (INT64_MAX + INT64_MIN = -1, ... + INT64_MIN + 1 wraps again), the expire's wrap back.  The gangs have their
    pod and all-zero MinResources, so PreFilter's own sums stay small."""
    L, N = 4, 3
    alloc = np.zeros((L, N), np.int64)
    alloc[0], alloc[1], alloc[2], alloc[3] = 1 << 62, 1 << 62, 1 << 40, 50
    reqd = np.zeros((L, N), np.int64)
    reqd[0, 0], reqd[1, 1] = I64MAX, I64MIN
    nodes = soa.Nodes(alloc, reqd, np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint8))
    fit = soa.FitMasks.from_bool(np.ones((1, N), bool))
    groups = soa.Groups.empty(2, L)
    groups.min_member[:] = 9
    groups.flags[:] = soa.GROUP_HAS_POD | soa.GROUP_HAS_MINRES
    group = np.array([0, 0, 1, 0, 1], np.int32)
    req = np.zeros((L, 5), np.int64)
    req[0] = [I64MIN, -5, I64MIN + 1, -1, 3]
    req[1] = [5, 0, 7, 0, I64MAX]
    pods = soa.Pods(group, req, np.zeros(5, np.uint32), np.zeros(5, np.uint32), np.zeros(5, np.uint64), np.zeros(5, np.uint8))
    with Case(bsa, soa, orc, (nodes, fit, groups, pods)) as c:
        assert c.st.wait_node.tolist() == [0, 0, 0, 0, -1] and int(c.st.requested[0, 0]) == I64MAX - 5
        c.expire("extremes, gang 1", groups=[1])
        assert int(c.st.requested[0, 0]) == -7                    # INT64_MAX - 5 - (INT64_MIN + 1) wraps
        c.expire("extremes, gang 0", groups=[0], deny=True)
        assert np.array_equal(c.st.requested, nodes.requested)
        c.follow_up("extremes")


# ---- flags and result caps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deny", [False, True])
def test_deny_closed_gang_and_earlier_entries(deny, bsa, soa, orc):
    scene = waiting_scene(soa, [4, 3, 5], n_nodes=3, matched0=[3, 0, 1], closed=(1,), interleave=True, seed=20)
    with Case(bsa, soa, orc, scene) as c:
        f = c.st.flags
        assert f[1] & soa.GROUP_PHASE_CLOSED and f[1] & soa.GROUP_SCHEDULED_LATCH and int((c.pods.group[c.st.wait_node >= 0] == 1).sum()) == 3
        e = c.expire(f"deny {deny}", groups=[1, 0], deny=deny)
        assert e["group_earlier"].tolist() == [0, 3] and e["group_pods"].tolist() == [3, 4]
        f = c.st.flags
        assert f[1] & soa.GROUP_PHASE_CLOSED and f[1] & soa.GROUP_SCHEDULED_LATCH and bool(f[1] & soa.GROUP_DENIED) == deny and not f[2] & soa.GROUP_DENIED
        c.follow_up(f"deny {deny}")


@pytest.mark.parametrize("pod_cap,group_cap", [(0, 0), (1, 1), (1, None)])
def test_result_caps(pod_cap, group_cap, bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [4, 3, 5], n_nodes=3, interleave=True, seed=21)) as c:
        assert int(np.isin(c.pods.group[c.st.wait_node >= 0], [1, 2]).sum()) == 8 > max(pod_cap, 1)   # more pods than the cap holds
        e = c.expire(f"caps {pod_cap} {group_cap}", groups=[2, 1], pod_cap=pod_cap, group_cap=group_cap)
        assert e["n_pods"] == 8 and e["n_groups"] == 2                 # (the true counts; check_state saw the state fully applied)
        c.follow_up("caps")


# ---- stages: against the object-level statement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ttl_writes", [False, True], ids=["filter", "filter+ttl-writes"])
@pytest.mark.parametrize("seed", [1001, 1002, 1003, 1004, 1005, 1006])
def test_filter_stage_passes_against_the_object_level(seed, ttl_writes, bsa, soa, orc):
    if seed % 2:
        sc, closed = _with_waiting(seed, n_nodes=int(4 + seed % 7), n_groups=int(2 + seed % 4), n_pods=int(20 + seed % 17), edge=False)
    else:
        sc, closed = _with_waiting(seed, n_nodes=int(3 + seed % 5), n_groups=3, n_pods=30, n_scalars=seed % 3, edge=True)
    stages = soa.STAGE_PREFILTER | soa.STAGE_FILTER | (soa.BATCH_FILTER_DENY if ttl_writes else 0)
    obj = sor.replay(sc, closed, run_filter=True, filter_deny=ttl_writes, scalar_names=sc["names"])
    nodes, fit, groups, pods, gidx = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], sc["denied"], sc["permitted"])
    for nm in closed:
        groups.flags[gidx[nm]] |= soa.GROUP_PHASE_CLOSED
    names = list(sc["cache"].keys())
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        r = ctx.seq_run(stages)
        assert r["pod_node"].tolist() == obj["pod_node"]
        op = obj["op"]
        uid_index = {pod.uid: i for i, pod in enumerate(sc["pods"])}
        want = np.full(pods.p, -1, np.int32)
        for nm in names:
            for uid, (node, _) in op.cache[nm].matched_pod_nodes.live(op.now).items():
                if uid in uid_index:
                    want[uid_index[uid]] = node
        assert np.array_equal(ctx.seq_waiting_read(), want)
        glist = [g for g in range(len(names)) if g % 2 == seed % 2] or [0]
        per = ser.expire_objects(op, sc, [names[g] for g in glist], deny=True, scalar_names=sc["names"])
        res = ctx.seq_expire(groups=glist, deny=True)
        assert res["group"].tolist() == glist and res["group_pods"].tolist() == [len(rows) for rows, _ in per]
        assert res["group_earlier"].tolist() == [e for _, e in per]
        assert list(zip(res["pod"].tolist(), res["node"].tolist())) == [x for rows, _ in per for x in rows]
        on = ser.object_nodes_soa(op, sc)
        req, pres = ctx.read_node_requests()
        assert np.array_equal(pres, on.requested_present) and np.array_equal(req[:4], on.requested[:4])
        for s in range(nodes.lanes - 4):
            has = ((pres >> s) & 1) != 0
            assert np.array_equal(req[4 + s][has], on.requested[4 + s][has])
        g = ctx.read_groups()
        assert g.matched.tolist() == [op.cache[nm].matched for nm in names]
        assert [bool(f & soa.GROUP_DENIED) for f in g.flags] == [op.last_denied.get(nm, op.now) is not None for nm in names]
        assert [bool(f & soa.GROUP_SCHEDULED_LATCH) for f in g.flags] == [bool(op.cache[nm].scheduled) for nm in names]


# ---- bs_seq_waiting_read -----------------------------------------------------------------------------------------------------------------
def test_waiting_read_before_partial_and_after_everything(bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [4, 3, 5], n_nodes=3, pods_cap=5, interleave=True, seed=30)) as c:
        w0 = c.ctx.seq_waiting_read()
        assert np.array_equal(w0, c.st.wait_node) and int((w0 >= 0).sum()) >= 4 and len(set(w0[w0 >= 0].tolist())) >= 2
        assert np.any(w0[c.pods.group == 1] >= 0) and np.any(w0[c.pods.group != 1] >= 0)
        c.expire("partial", groups=[1])
        w1 = c.ctx.seq_waiting_read()
        assert np.all(w1[c.pods.group == 1] == -1) and np.array_equal(w1[c.pods.group != 1], w0[c.pods.group != 1])
        c.expire("everything", all=True)
        assert np.all(c.ctx.seq_waiting_read() == -1)
        buf = np.zeros(c.pods.p + 1, np.int32)                     # p must be the queue length
        for p in (c.pods.p + 1, c.pods.p - 1):
            assert status_of(bsa, lambda: c.ctx._chk(c.ctx._lib.bs_seq_waiting_read(c.ctx._h, p, buf.ctypes.data_as(bsa.capi.C.POINTER(bsa.capi.C.c_int32))),
                                                     "bs_seq_waiting_read")) == -1
        c.follow_up("waiting reads")


# ---- the validity window -----------------------------------------------------------------------------------------------------------------
def _node_delta(bsa, case, kind, index):
    d = bsa.capi.NodeDelta()
    d.kind, d.index = kind, index
    for j in range(case.nodes.lanes):
        d.allocatable[j] = int(case.nodes.allocatable[j, 0])
        d.requested[j] = 0
    d.allocatable_present, d.requested_present, d.flags, d.fit_default, d.n_fit_exceptions = int(case.nodes.allocatable_present[0]), 0, 0, 1, 0
    return d


ENDERS = ["pods_load", "pods_apply", "nodes_load", "nodes_append", "nodes_remove", "groups_load"]


@pytest.mark.parametrize("ender", ENDERS)
def test_calls_that_end_the_window(ender, bsa, soa, orc):
    capi = bsa.capi
    with Case(bsa, soa, orc, waiting_scene(soa, [3, 2], n_nodes=3, seed=40)) as c:
        ctx = c.ctx
        {"pods_load": lambda: ctx.load_pods(c.pods),
         "pods_apply": lambda: ctx.apply_pods(flag_index=[0], flag_value=[0]),
         "nodes_load": lambda: (ctx.load_nodes(c.model_nodes(), c.fit)),
         "nodes_append": lambda: ctx.apply_node_deltas([_node_delta(bsa, c, capi.DELTA_APPEND, 0)]),
         "nodes_remove": lambda: ctx.apply_node_deltas([_node_delta(bsa, c, capi.DELTA_REMOVE, 2)]),
         "groups_load": lambda: ctx.load_groups(c.model_groups())}[ender]()
        assert status_of(bsa, lambda: ctx.seq_expire(all=True)) == -4
        assert status_of(bsa, lambda: ctx.seq_expire(groups=[0])) == -4
        assert status_of(bsa, lambda: ctx.seq_waiting_read()) == -4
        if ender in ("pods_load", "pods_apply", "groups_load"):   # the next pass opens a new window
            ctx.seq_run(soa.STAGE_PREFILTER)
            ctx.seq_waiting_read()
            ctx.seq_expire(all=True)


def test_before_any_pass_and_on_a_sharded_context(bsa, soa, orc):
    nodes, fit, groups, pods = waiting_scene(soa, [3, 2], n_nodes=3, seed=41)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        assert status_of(bsa, lambda: ctx.seq_expire(all=True)) == -4
        assert status_of(bsa, lambda: ctx.seq_waiting_read()) == -4
        ctx.seq_run(soa.STAGE_PREFILTER)
        ctx.set_shard(0, 2)
        assert status_of(bsa, lambda: ctx.seq_expire(all=True)) == -4
        assert status_of(bsa, lambda: ctx.seq_waiting_read()) == -4
        ctx.set_shard(0, 1)
        assert ctx.seq_expire(all=True)["n_pods"] == 5


def test_calls_that_leave_the_window_open(bsa, soa, orc):
    """bs_nodes_assume on a touched node, a bs_nodes_apply of UPDATEs, bs_groups_apply and a batch in between: the result is
    model(pass) + those calls - the forgotten pods"""
    capi = bsa.capi
    with Case(bsa, soa, orc, waiting_scene(soa, [4, 3, 5], n_nodes=3, S=1, pods_cap=6, interleave=True, seed=42)) as c:
        ctx, st = c.ctx, c.st
        k = int(st.wait_node[0])
        lanes = (st.requested[:, k] + np.array([500, 1 << 20, 3, 2, 1])).tolist()
        ctx.assume_nodes([(k, lanes, int(st.requested_present[k]) | 1)])
        st.requested[:, k] = lanes
        st.requested_present[k] |= 1
        c.check_state("after bs_nodes_assume")
        k2 = int(st.wait_node.max())
        assert k2 != k
        d = _node_delta(bsa, c, capi.DELTA_UPDATE, k2)
        for j in range(5):
            d.allocatable[j] = int(c.nodes.allocatable[j, k2])
            d.requested[j] = int(st.requested[j, k2]) + 11
        d.allocatable_present, d.requested_present = int(c.nodes.allocatable_present[k2]), int(st.requested_present[k2])
        ctx.apply_node_deltas([d])
        st.requested[:, k2] += 11
        c.check_state("after bs_nodes_apply(UPDATE)")
        ctx.apply_group_deltas([(2, int(st.matched[2]) + 2, 1, int(st.flags[2]))])
        st.matched[2] += 2
        c.mg.status_scheduled[2] = 1
        c.check_state("after bs_groups_apply")
        ctx.batch(soa.STAGE_ALL, bitmap=False)
        e = c.expire("after assume / update / groups_apply / batch", groups=[2, 0], deny=True)
        assert e["group_earlier"].tolist() == [2, 0]
        c.expire("the rest", all=True)
        c.follow_up("calls that leave the window open")


def _move(st, k, req, pres, S, sign):
    """NodeInfo.AddPod (sign +1) / RemovePod (-1) of one pod on node k of the model, by the rule k_pc_nodes and k_ba_nodes state: a scalar lane
    the pod has starts from 0 where the node lacks the key, and the node's bit is set"""
    for j in range(3):
        st.requested[j, k] = ser.w64(int(st.requested[j, k]) + sign * int(req[j]))
    st.requested[3, k] = ser.w64(int(st.requested[3, k]) + sign)
    for s in range(S):
        if (int(pres) >> s) & 1:
            base = int(st.requested[4 + s, k]) if (int(st.requested_present[k]) >> s) & 1 else 0
            st.requested[4 + s, k] = ser.w64(base + sign * int(req[4 + s]))
            st.requested_present[k] |= np.uint32(1 << s)


def _preempt_scene(soa):
    """five waiting pods of two gangs on node 1 (node 0 is unschedulable), a node 1 that is nearly full of cpu, three bound pods on it, and
    two ungrouped pods at the queue's end that found no node in the pass: the preemptors (fit class 1: node 1 only)"""
    nodes, fit, groups, pods = waiting_scene(soa, [3, 2], n_nodes=3, S=1, skip_nodes=1, interleave=True, seed=50)
    nodes.requested[0] += 6_000_000
    fit = soa.FitMasks.from_bool(np.array([[True, True, True], [False, True, False]]))
    big = soa.Pods.empty(2, 5)
    big.group[:] = soa.POD_NOT_GROUPED
    big.req[0] = [4_500_000, 4_200_000]
    big.req[4], big.req_present[:], big.cls[:] = [1, 0], [1, 0], 1
    pods = soa.Pods(*[np.concatenate([getattr(pods, f), getattr(big, f)], axis=-1) for f in ("group", "req", "req_present", "cls", "owner", "flags")])
    bound = soa.Bound.empty(4, 5)
    bound.node[:] = [1, 1, 1, 2]
    bound.priority[:] = [0, 0, 5000, 0]
    bound.start_ns[:] = [10, 20, 30, 40]
    bound.req[0] = [3_500_000, 2_400_000, 100, 7]
    bound.req[4], bound.req_present[:] = [0, 3, 2, 0], [0, 1, 1, 0]
    return (nodes, fit, groups, pods), bound


def test_preemption_and_bound_table_calls_leave_the_window_open(bsa, soa, orc):
    """bs_preempt_commit(APPLY | ASSUME), bs_preempt_commit_gang(APPLY), bs_bound_apply_ex(BS_BOUND_NODES) and an UPDATE-only
    bs_nodes_apply + bs_bound_nodes_apply on the node the waiting pods sit on, between the pass and the expire: each writes the node
    requests and the host mirror through its own records, and the expire is model(pass) + those deltas - the forgotten pods; a
    bs_nodes_apply(UPDATE) of ANOTHER node afterwards re-uploads the list from the host mirror, which must therefore be right"""
    capi = bsa.capi
    scene, bound = _preempt_scene(soa)
    with Case(bsa, soa, orc, scene) as c:
        ctx, st, pods, P = c.ctx, c.st, c.pods, c.pods.p
        assert np.all(st.wait_node[:5] == 1) and np.all(st.wait_node[5:] == -1) and np.all(c.s["pod_node"][5:] == -1) and np.all(c.s["pf_code"][5:] < 16)
        ctx.load_bound(bound)
        prot = np.zeros(2, np.uint8)
        r = ctx.preempt_commit([P - 2], [1000], prot, victim_cap=4, apply=True, assume=True)
        assert r["node"].tolist() == [1] and r["n_victims"].tolist() == [1] and int(r["victims"][0, 0]) in (0, 1)
        v = int(r["victims"][0, 0])
        _move(st, 1, bound.req[:, v], bound.req_present[v], 1, -1)
        _move(st, 1, pods.req[:, P - 2], pods.req_present[P - 2], 1, +1)
        c.check_state("after bs_preempt_commit(APPLY | ASSUME)")
        r = ctx.preempt_commit_gang([P - 1], [1000], prot, gang_need=np.zeros(2, np.uint32), victim_cap=4, apply=True)
        assert r["node"].tolist() == [1] and r["n_victims"].tolist() == [1] and int(r["victims"][0, 0]) == 1 - v
        _move(st, 1, bound.req[:, 1 - v], bound.req_present[1 - v], 1, -1)
        c.check_state("after bs_preempt_commit_gang(APPLY)")
        ins = soa.Bound.empty(1, 5)
        ins.node[:], ins.priority[:], ins.start_ns[:] = 1, 7, 50
        ins.req[0], ins.req[4], ins.req_present[:] = 77, 5, 1
        ctx.bound_apply_ex(remove=[2], insert=ins)
        _move(st, 1, bound.req[:, 2], bound.req_present[2], 1, -1)
        _move(st, 1, ins.req[:, 0], ins.req_present[0], 1, +1)
        c.check_state("after bs_bound_apply_ex(BS_BOUND_NODES)")
        c.expire("after the preemption and bound-table calls", groups=[1], deny=True)
        d = _node_delta(bsa, c, capi.DELTA_UPDATE, 0)                  # node 0 as it is: the upload behind it comes from the host mirror
        for j in range(5):
            d.allocatable[j], d.requested[j] = int(c.nodes.allocatable[j, 0]), int(st.requested[j, 0])
        d.allocatable_present, d.requested_present, d.flags, d.fit_default = int(c.nodes.allocatable_present[0]), int(st.requested_present[0]), int(c.nodes.flags[0]), 0
        d.n_fit_exceptions, d.fit_exceptions[0] = 1, 0
        ctx.apply_node_deltas([d])
        c.check_state("after bs_nodes_apply(UPDATE) from the mirror")
        ctx.bound_nodes_apply([capi.DELTA_UPDATE], [0])               # follows UPDATEs only: no renumbering, the window stays open
        c.check_state("after bs_bound_nodes_apply(UPDATE)")
        e = c.expire("the other gang", all=True)
        assert e["group"].tolist() == [0] and e["n_pods"] == 3
        c.follow_up("preemption and bound-table calls")


@pytest.mark.parametrize("kind", ["append", "remove"])
def test_bound_nodes_apply_does_not_reopen_a_window_the_surgery_ended(kind, bsa, soa, orc):
    """bs_nodes_apply with an APPEND or a REMOVE ends the window; the bs_bound_nodes_apply that follows it neither ends nor reopens one"""
    capi = bsa.capi
    scene, bound = _preempt_scene(soa)
    with Case(bsa, soa, orc, scene) as c:
        ctx = c.ctx
        ctx.load_bound(bound)
        k, idx = (capi.DELTA_APPEND, 0) if kind == "append" else (capi.DELTA_REMOVE, 2)
        ctx.apply_node_deltas([_node_delta(bsa, c, k, idx)])
        assert status_of(bsa, lambda: ctx.seq_expire(all=True)) == -4
        ctx.bound_nodes_apply([k], [idx])
        assert status_of(bsa, lambda: ctx.seq_expire(all=True)) == -4 and status_of(bsa, lambda: ctx.seq_waiting_read()) == -4


def test_every_invalid_argument_leaves_the_state_alone(bsa, soa, orc):
    with Case(bsa, soa, orc, waiting_scene(soa, [3, 2, 2], n_nodes=3, seed=43)) as c:
        ctx, lib = c.ctx, c.ctx._lib
        for where, fn in [("index >= g", lambda: ctx.seq_expire(groups=[0, 3])),
                          ("listed twice", lambda: ctx.seq_expire(groups=[1, 0, 1])),
                          ("NULL list without ALL", lambda: ctx.seq_expire(groups=None)),
                          ("NULL list with a count", lambda: ctx._chk(lib.bs_seq_expire(ctx._h, 2, None, 0, bsa.capi.SeqExpireOut()), "bs_seq_expire")),
                          ("ALL with a list", lambda: ctx.seq_expire(groups=[0], all=True)),
                          ("unknown flag bits", lambda: ctx.seq_expire(groups=[0], flags=4)),
                          ("unknown flag bits with ALL", lambda: ctx.seq_expire(flags=2 | 0x80000000)),
                          ("NULL result array", lambda: ctx._chk(lib.bs_seq_expire(ctx._h, 0, None, 2, bsa.capi.SeqExpireOut(0, 0, 1, None, None, None, 0, None, None)), "bs_seq_expire")),
                          ("NULL out", lambda: ctx._chk(lib.bs_seq_expire(ctx._h, 0, None, 2, None), "bs_seq_expire"))]:
            assert status_of(bsa, fn) == -1, where
            c.check_state(f"after the refused call: {where}")
        assert c.ctx.seq_expire(groups=[])["n_groups"] == 0       # an empty list is no error and no change
        c.check_state("after an empty list")
        c.expire("and the state still expires", all=True)
        c.follow_up("refused calls")


# ---- fuzz ----------------------------------------------------------------------------------------------------------------------------------
def test_fuzz_passes_expires_assumes_group_patches_queue_patches_batches(bsa, soa, orc):
    rng = np.random.default_rng(2026)
    sc, closed = _with_waiting(8, n_nodes=6, n_groups=6, n_pods=60, n_scalars=2, edge=False)
    nodes, fit, groups, pods, gidx = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], sc["denied"], sc["permitted"])
    nodes.requested[:3] = nodes.requested[:3] // 4                 # room: gangs do get nodes
    nodes.requested[3] = np.minimum(nodes.requested[3], 5)
    for nm in closed:
        groups.flags[gidx[nm]] |= soa.GROUP_PHASE_CLOSED
    G, N = groups.g, nodes.n
    keep = soa.GROUP_HAS_POD | soa.GROUP_HAS_MINRES
    st, mg, valid, n_exp, n_state = None, groups.copy(), False, 0, 0
    req, pres = nodes.requested.copy(), nodes.requested_present.copy()
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        for step in range(60):
            where = f"step {step}"
            op = "pass" if step == 0 else rng.choice(["pass", "expire", "expire", "expire_all", "assume", "groups", "pods", "batch"])
            cur = soa.Nodes(nodes.allocatable, req, nodes.allocatable_present, pres, nodes.flags)
            if op == "pass":
                s = orc.seq_replay(cur, fit, mg, pods, soa.STAGE_PREFILTER)
                r = ctx.seq_run(soa.STAGE_PREFILTER)
                assert np.array_equal(r["pf_code"], s["pf_code"]) and np.array_equal(r["pod_node"], s["pod_node"]), where
                st = ser.State.after_pass(cur, fit, mg, pods, s)
                mg, req, pres, valid = s["groups"].copy(), st.requested, st.requested_present, True
            elif op in ("expire", "expire_all"):
                lst = None if op == "expire_all" else rng.permutation(G)[: int(rng.integers(0, G + 1))]
                deny = bool(rng.integers(0, 2))
                if not valid:
                    assert status_of(bsa, lambda: ctx.seq_expire(groups=lst, deny=deny, all=lst is None)) == -4, where
                    n_state += 1
                else:
                    st.matched, st.flags = mg.matched, mg.flags
                    exp = ser.expire(st, pods, groups=lst, deny=deny, all=lst is None)
                    res = ctx.seq_expire(groups=lst, deny=deny, all=lst is None)
                    for k in ("n_groups", "n_pods", "group", "group_pods", "group_earlier", "pod", "node"):
                        assert np.array_equal(res[k], exp[k]), f"{where}: {k}"
                    n_exp += exp["n_pods"]
            elif op == "assume":
                k = int(rng.integers(0, N))
                req[:, k] += rng.integers(0, 3, nodes.lanes)
                ctx.assume_nodes([(k, req[:, k].tolist(), int(pres[k]))])
            elif op == "groups":
                g = int(rng.integers(0, G))
                mg.matched[g] = int(rng.integers(0, 3))
                mg.flags[g] = (int(mg.flags[g]) & keep) | int(rng.choice([0, soa.GROUP_DENIED, soa.GROUP_SCHEDULED_LATCH]))
                ctx.apply_group_deltas([(g, int(mg.matched[g]), int(mg.status_scheduled[g]), int(mg.flags[g]))])
            elif op == "pods":
                gone = rng.permutation(pods.p)[: int(rng.integers(1, 4))] if pods.p > 8 else np.zeros(0, np.int64)
                ctx.apply_pods(remove=np.sort(gone).astype(np.uint32))
                pods = pods.take(np.setdiff1d(np.arange(pods.p), gone))
                valid = False
            else:
                got = ctx.batch(soa.STAGE_ALL, bitmap=False)
                exp = orc.Sop(orc.Snapshot(cur, fit), mg).batch(pods, soa.STAGE_ALL, bitmap=False)
                for name in ("pf_code", "pf_first_k", "fl_code", "fl_feasible", "group_admit", "group_ready"):
                    assert np.array_equal(getattr(got, name), getattr(exp, name)), f"{where}: batch {name}"
            q, p_ = ctx.read_node_requests()
            assert np.array_equal(q, req) and np.array_equal(p_, pres), f"{where} ({op}): node requests"
            assert_groups_equal(ctx.read_groups(), mg, soa, f"{where} ({op})")
            if valid:
                assert np.array_equal(ctx.seq_waiting_read(), st.wait_node), f"{where} ({op}): waiting state"
    assert n_exp >= 5 and n_state >= 1, (n_exp, n_state)
