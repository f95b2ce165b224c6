"""Scenes for bs_seq_run_scored (TEST INFRASTRUCTURE), for tests/test_seq_scored_cpu.py and tests/test_gpu_seq_scored.py: seeded random object
scenes on the generator the nominated pass's scenes use (scenarios.random_objects, pods from a few templates, room made on the nodes), and
scenes built node by node — identical nodes, lanes outside rule P's domain, and the geometry of the kernel's tile walk (thread t of the
512-thread block votes for tile chunk + t of 64 nodes; wave w visits tiles 64 w .. 64 w + 63 of a chunk of 32 768 nodes).  The CPU tests
assert that these very scenes meet every hazard of the model."""
import json
import os

import numpy as np

import naive_ref as nv
import scenarios

GI = 1 << 30
I64_MAX = (1 << 63) - 1
NAMES12 = [f"example.com/r{i}" for i in range(12)]
WEIGHTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (3, 2, 1)]
EDGE_N = [1, 63, 64, 65, 130, 8 * 64 - 1, 8 * 64, 8 * 64 + 1]
# the model's full comparison with zero weights, and the hazard census, run over these
SEEDS = list(range(9100, 9124))
# the GPU parity set: (seed, nodes, scalar lanes, gangs); 4 lanes is the last count at which the kernel keeps everything in registers
PARITY = [(9100 + i, EDGE_N[i % 8], (0, 1, 4)[i % 3], i % 4 != 3) for i in range(16)]
# ... and the same at the maximum lane count of a context (BS_MAX_SCALARS), and at the first and a middle one of the kernel's lean form
PARITY_MAX = [(9130, 130, 12, True), (9131, 65, 12, False), (9132, 8 * 64 + 1, 12, True), (9133, 63, 5, True), (9134, 130, 9, False)]
FILTER_SEEDS = list(range(9100, 9110))                           # the BS_STAGE_FILTER family (filter_scene)
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_scored_hand_kats.json")


def make(seed, n_nodes=48, n_groups=8, n_pods=120, n_scalars=None, gangs=True, room=0.6, edge=None, tight=False, spice=None):
    """a random scene: pods from six templates (request classes repeat, as a gang's do), node utilisation scaled into [0, room).
    gangs=False: every pod is ungrouped.  tight: pod counts near the allocatable, so that C is small and the choice matters early."""
    rng = np.random.default_rng(seed ^ 0x5C0)
    S = seed % 3 if n_scalars is None else n_scalars
    saved = scenarios.SCALARS
    scenarios.SCALARS = NAMES12 if S > 2 else saved
    try:
        sc = scenarios.random_objects(seed, n_nodes=n_nodes, n_groups=n_groups, n_pods=n_pods, n_scalars=S, n_classes=3,
                                      edge=(seed % 5 == 4) if edge is None else edge)
    finally:
        scenarios.SCALARS = saved
    templates = [dict(p.requests) for p in sc["pods"][:6]]
    for p in sc["pods"]:
        p.requests = dict(templates[int(rng.integers(0, len(templates)))])
        if not gangs:
            p.group = None
    for info in sc["nodes"]:
        u = rng.uniform(0.0, room)
        r = info.requested
        r.MilliCPU, r.Memory, r.EphemeralStorage = int(r.MilliCPU * u), int(r.Memory * u), int(r.EphemeralStorage * u)
        back = int(rng.integers(1, 4)) if tight else int(rng.integers(1, 30))
        info.pod_count = int(min(info.pod_count, max(info.allocatable.AllowedPodNumber - back, 0)))
    if seed % 2 if spice is None else spice:
        # lanes outside rule P's domain on nodes that still hold pods (a negative requested value, an allocatable of 2^53 and beyond), and
        # nodes that a template's request fills to the brim (R == A: least 0, balanced 0)
        for info in sc["nodes"]:
            x = rng.random()
            if x < 0.06:
                info.requested.MilliCPU = -int(rng.integers(1, 5000))
            elif x < 0.10:
                info.allocatable.Memory = (1 << 53) + int(rng.integers(0, 3)) - 1
            elif x < 0.13:
                info.allocatable.MilliCPU = I64_MAX - int(rng.integers(0, 2))
            elif x < 0.25:
                t = templates[int(rng.integers(0, len(templates)))]
                info.requested.MilliCPU = info.allocatable.MilliCPU - int(rng.integers(1, 4)) * t["cpu"]
    return sc


def parity_scene(seed, n, S, gangs):
    return make(seed, n_nodes=n, n_groups=8 if gangs else 1, n_pods=min(200, 60 + 2 * n), n_scalars=S, gangs=gangs)


def filter_scene(seed, n=40):
    """the family for BS_STAGE_FILTER: few nodes, many gangs with MinResources, so that computeResourceSatisfied is evaluated on every
    node for most pods and turns nodes away (hazard i of the model)"""
    return make(seed, n_nodes=n, n_groups=10, n_pods=90, n_scalars=seed % 2, room=0.9, edge=False)


def _node(cpu, mem, rcpu=0, rmem=0, pods=110, **kw):
    a, r = nv.Resource(), nv.Resource()
    a.Add({"cpu": cpu, "memory": mem, "pods": pods})
    r.MilliCPU, r.Memory = rcpu, rmem
    return nv.NodeInfo(a, r, 0, **kw)


def _scene(nodes, pods, cache=None):
    return dict(nodes=nodes, cache=cache or {}, pods=pods, names=[], n_classes=1, denied=set(), permitted=set())


def identical(n=8, p=20):
    """identical empty nodes of 4000 mCPU / 8 GiB and identical ungrouped pods of 500 mCPU / 1 GiB: (1, 0, 1) spreads, (0, 1, 0) packs"""
    return _scene([_node(4000, 8 * GI) for _ in range(n)], [nv.Pod(f"uid{i}", None, {"cpu": 500, "memory": GI}) for i in range(p)])


def out_of_domain():
    """nodes that hold the pod with a lane outside rule P's domain, between ordinary ones: allocatable 0 (the pod asks for no cpu), allocatable
    2^53 and INT64_MAX, a negative requested value, and a sum requested + request that wraps (a negative request on a requested value at the
    bottom of int64).  They score 0 on that lane and compete on what is left, in the end on the index."""
    nodes = [
        _node(0, 8 * GI),                                        # 0: A = 0 on cpu
        _node(4000, 8 * GI, 3000, 6 * GI),                       # 1: ordinary, rather full
        _node(1 << 53, 8 * GI),                                  # 2: A = 2^53 on cpu: one past the domain
        _node((1 << 53) - 1, 8 * GI),                            # 3: the largest A inside
        _node(4000, 8 * GI, -500, 0),                            # 4: negative requested: R < 0
        _node(4000, I64_MAX, 0, 0),                              # 5: A = INT64_MAX on memory
        _node(4000, 8 * GI, -(1 << 63) + 50, 0),                 # 6: requested + request wraps to 2^63 - 50 for the pod that asks for -100
        _node(4000, 8 * GI, 1000, 2 * GI),                       # 7: ordinary, rather empty
        _node(0, 0),                                             # 8: both lanes out (the pods ask for no cpu; memory does not fit)
    ]
    pods = []
    for i in range(18):
        rq = ({"cpu": 0, "memory": GI}, {"cpu": 0, "memory": 2 * GI}, {"cpu": -100, "memory": GI}, {"cpu": 0, "memory": 0})[i % 4]
        pods.append(nv.Pod(f"uid{i}", None, dict(rq)))
    return _scene(nodes, pods)


WALK = 512 * 64                                                  # nodes of one tile walk of the 512-thread block


def geometry_walks():
    """N = 32 768 + 70, six ungrouped pods of 1000 mCPU / 1 GiB.  Every node is full but three: the last lane of the last tile of the first
    walk (32 767), lane 0 of the first tile of the second walk (32 768) and the last valid node (32 837).  The first two are identical — a
    tie across the two walks that the lower index wins —, the third is larger, so it wins while it is emptier."""
    n = WALK + 70
    nodes = [_node(4000, 8 * GI, 4000, 0) for _ in range(n)]
    nodes[WALK - 1] = _node(4000, 8 * GI, 0, 0)
    nodes[WALK] = _node(4000, 8 * GI, 0, 0)
    nodes[n - 1] = _node(6000, 12 * GI, 0, 0)
    return _scene(nodes, [nv.Pod(f"uid{i}", None, {"cpu": 1000, "memory": GI}) for i in range(6)])


def geometry_waves():
    """N = 4096 + 300: tiles 64 .. 68 belong to wave 1.  Candidates: lane 5 of tile 64 and lane 5 of tile 65 (one lane of wave 1 sees both; the
    second is the better one), lanes 1 and 9 of tile 66 (a tie inside one tile) and lane 0 of tile 2 (wave 0, the first fit, the worst)."""
    n = 4096 + 300
    nodes = [_node(4000, 8 * GI, 4000, 0) for _ in range(n)]
    nodes[2 * 64] = _node(4000, 8 * GI, 2500, 5 * GI)
    nodes[64 * 64 + 5] = _node(4000, 8 * GI, 1000, 2 * GI)
    nodes[65 * 64 + 5] = _node(4000, 8 * GI, 500, GI)
    nodes[66 * 64 + 1] = _node(4000, 8 * GI, 500, GI)
    nodes[66 * 64 + 9] = _node(4000, 8 * GI, 500, GI)
    return _scene(nodes, [nv.Pod(f"uid{i}", None, {"cpu": 500, "memory": GI}) for i in range(6)])


def to_soa(sc):
    """(nodes, fit, groups, pods, owner_ids) of a scene: what the device is loaded with"""
    owner_ids = {}
    nodes, fit, groups, pods, _ = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], denied=sc["denied"], permitted=sc["permitted"],
                                            owner_ids=owner_ids)
    return nodes, fit, groups, pods, owner_ids


# ---- the hand-derived file ---------------------------------------------------------------------------------------------------------------------
def load_kats():
    return json.load(open(KATS))


def kat_scene(k: dict):
    """a three-node scene of the golden file as objects"""
    nodes = [_node(nd["alloc"][0], nd["alloc"][1], nd["req"][0], nd["req"][1]) for nd in k["nodes"]]
    return _scene(nodes, [nv.Pod(f"uid{i}", None, {"cpu": p[0], "memory": p[1]}) for i, p in enumerate(k["pods"])])
