"""Scenes for bs_seq_run_nominated (TEST INFRASTRUCTURE): random object scenes with a nominated-pod table shaped so that rule S decides
something — rows on the first-fit front (the nodes the row-less pass fills), priorities drawn around the queue's, some queue pods that own a
row — and the hand-derived scenes of tests/golden/seq_nominated_hand_kats.json as objects.  The CPU tests assert the non-vacuity of the very
set the GPU tests run (tests/test_seq_nominated_cpu.py)."""
import json
import os

import numpy as np

import naive_ref as nv
import scenarios
import seq_nominated_ref as snr

GI = 1 << 30
PRIOS = (0, 10, 20, 30)
# the GPU parity set: (seed, nodes, rows); >= 40 seeds, N in {48, 130, 200}, m in {1, 7, 64, 300}
PARITY = [(5200 + i, (48, 130, 200)[i % 3], (7, 64, 300, 1)[i % 4]) for i in range(42)]
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_nominated_hand_kats.json")


def _row_req(pod_req: dict, names) -> nv.Resource:
    r = nv.Resource()
    r.Add({k: v for k, v in pod_req.items() if k != "pods"})
    r.AllowedPodNumber = 1
    r.ScalarResources = {k: v for k, v in (r.ScalarResources or {}).items() if k in names} or None
    return r


def make(seed, n_nodes=48, m=64, n_groups=10, n_pods=140, first_open=0, row_nodes=(), own_pods=None, own_rows=None, n_scalars=None, names=None):
    """-> dict(sc, names, priority [p], own_id [p], nominees [m] in id order, rowless: the model's pass without a table).
    The edge scenes: first_open: the nodes in front of it are unschedulable (the first-fit front starts there); row_nodes: nodes the last
    rows are put on, each asking most of the node at the top priority; own_pods / own_rows: queue indices that own a row, and those rows'
    ids (the pods get the top priority, so that they are placed and their rows consumed); names: the scalar names to draw from."""
    rng = np.random.default_rng(seed ^ 0x5E9)
    saved = scenarios.SCALARS
    scenarios.SCALARS = list(names) if names is not None else saved
    try:
        sc = scenarios.random_objects(seed, n_nodes=n_nodes, n_groups=n_groups, n_pods=n_pods, n_scalars=seed % 3 if n_scalars is None else n_scalars,
                                      n_classes=3, edge=(seed % 5 == 4))
    finally:
        scenarios.SCALARS = saved
    names = sc["names"]
    templates = [dict(p.requests) for p in sc["pods"][:6]]      # pods come from a few templates, as a gang's do: request classes repeat,
    for p in sc["pods"]:                                        # which is what the first-fit cursors are keyed by
        p.requests = dict(templates[int(rng.integers(0, len(templates)))])
    for k in range(first_open):
        sc["nodes"][k].unschedulable = True
    for info in sc["nodes"]:                                    # make room (the raw scenes are 0-110 % utilised)
        u = rng.uniform(0.0, 0.6)
        r = info.requested
        r.MilliCPU, r.Memory, r.EphemeralStorage = int(r.MilliCPU * u), int(r.Memory * u), int(r.EphemeralStorage * u)
        info.pod_count = int(min(info.pod_count, max(info.allocatable.AllowedPodNumber - int(rng.integers(1, 30)), 0)))
    P = len(sc["pods"])
    priority = np.array([PRIOS[int(rng.integers(0, len(PRIOS)))] for _ in range(P)], np.int32)
    if own_pods is not None:
        priority[list(own_pods)] = 40
    rowless = snr.replay(sc, [], priority, None, scalar_names=names)
    front = sorted({k for k in rowless["assumed"] if k >= 0}) or list(range(min(4, n_nodes)))
    if own_pods is None:
        n_own = min((m + 1) // 3, 20, P)
        own_pods = rng.choice(P, size=n_own, replace=False) if n_own else np.zeros(0, np.int64)
    own_rows = list(range(len(own_pods))) if own_rows is None else list(own_rows)
    assert len(own_rows) == len(own_pods) and all(r < m for r in own_rows)
    n_own = len(own_rows)
    own_id = np.full(P, snr.NOM_NONE, np.uint32)
    nominees = []
    for r in range(m):
        if r in own_rows:                                       # the row IS a queue pod: its request, its priority
            i = int(own_pods[own_rows.index(r)])
            at = rowless["assumed"][i]
            node = at if at >= 0 and rng.random() < 0.5 else int(rng.choice(front))
            nominees.append(snr.Nominee(r, int(node), int(priority[i]), _row_req(sc["pods"][i].requests, names)))
            own_id[i] = r
            continue
        node = int(rng.choice(front)) if rng.random() < 0.8 else int(rng.integers(0, n_nodes))
        info = sc["nodes"][node]
        free = max(info.allocatable.MilliCPU - info.requested.MilliCPU, 0)
        rq = {"cpu": int(free * rng.uniform(0.3, 1.0)), "memory": int(rng.choice([0, 1, 2])) * GI}
        for nm in names:
            if rng.random() < 0.4:
                rq[nm] = int(rng.choice([1, 2, 8]))
        prio = PRIOS[int(rng.integers(0, len(PRIOS)))] + int(rng.choice([-1, 0, 0, 1]))
        nominees.append(snr.Nominee(r, node, prio, _row_req(rq, names)))
    others = [r for r in range(m) if r not in own_rows]
    for node, r in zip(row_nodes, reversed(others)):
        a = sc["nodes"][node].allocatable
        nominees[r] = snr.Nominee(r, int(node), 35, nv.Resource(int(a.MilliCPU * 0.9), 0, 0, 1, None))
    if seed % 6 == 5 and m >= 2 + n_own and not row_nodes and own_rows == list(range(n_own)):                        # sums that wrap int64: two rows of 2^63 - 1 add up to -2
        for r in (m - 2, m - 1):
            nominees[r] = snr.Nominee(r, front[0], 15, nv.Resource((1 << 63) - 1, 0, 0, 1, None))
    return dict(sc=sc, names=names, priority=priority, own_id=own_id, nominees=nominees, rowless=rowless)


def parity_scene(seed, n, m):
    """a scene of the PARITY set.  With 130 and 200 nodes the first-fit front starts a few nodes in front of a tile border (node 64, node
    128), so that it straddles two tiles of 64 nodes: the kernel's cursors are per tile, and a cursor hazard shows only across tiles"""
    return make(seed, n_nodes=n, m=m, first_open={48: 0, 130: 56, 200: 120}[n])


def to_soa(scn):
    """(nodes, fit, groups, pods, owner_ids, rows) of a scene: what the device is loaded with"""
    sc, owner_ids = scn["sc"], {}
    nodes, fit, groups, pods, _ = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], denied=sc["denied"], permitted=sc["permitted"],
                                            owner_ids=owner_ids)
    return nodes, fit, groups, pods, owner_ids, snr.objects_to_rows(scn["nominees"], scn["names"])


# ---- the hand-derived scenes -------------------------------------------------------------------------------------------------------------
def load_kats():
    return json.load(open(KATS))["scenes"]


def kat_scene(k: dict, names=None):
    """one scene of the golden file as objects (names: the context's scalar names; default: the scene's own)"""
    names = list(k.get("scalars", [])) if names is None else list(names)
    assert set(k.get("scalars", [])) <= set(names)
    nodes = []
    full = {"alloc": {"cpu": 4000, "memory": 64 * GI, "pods": 10}, "req": {"cpu": 4000}}
    for nd in [x for e in k["nodes"] for x in ([full] * e["full"] if "full" in e else [e])]:
        a, r = nv.Resource(), nv.Resource()
        a.Add(nd["alloc"])
        r.Add(nd.get("req", {}))
        nodes.append(nv.NodeInfo(a, r, 0, unschedulable=bool(nd.get("unschedulable", False))))
    cache = {g["name"]: nv.PGS(nv.PodGroup(g["name"], g["min_member"])) for g in k.get("groups", [])}
    pods = [nv.Pod(f"uid{i}", p.get("group"), dict(p["req"])) for i, p in enumerate(k["pods"])]
    sc = dict(nodes=nodes, cache=cache, pods=pods, names=names, n_classes=1, denied=set(k.get("denied", [])), permitted=set())
    priority = np.array([p["priority"] for p in k["pods"]], np.int32)
    own_id = np.array([snr.NOM_NONE if p.get("own") is None else p["own"] for p in k["pods"]], np.uint32)
    nominees = [snr.Nominee(i, r["node"], r["priority"], _row_req(r["req"], names)) for i, r in enumerate(k["rows"])]
    return dict(sc=sc, names=names, priority=priority, own_id=own_id, nominees=nominees, rowless=None)
