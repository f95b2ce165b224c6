"""Scenes for bs_seq_run_scored_nominated (TEST INFRASTRUCTURE), for tests/test_seq_scored_nominated_cpu.py and
tests/test_gpu_seq_scored_nominated.py: seq_nominated_scenes.make (a table with rows on the front, queue pods that own rows) composed with the
spice of seq_scored_scenes.make (lanes outside rule P's domain, nodes a template fills to the brim), and the rows moved to where rule SP can
decide something: onto the nodes the table-less SCORED pass fills, in sizes from a sliver of the free cpu (the row is seen and does not
block: D8 shows) to all of it (the row blocks: the maximum is turned away).  The hand-derived scenes of
tests/golden/seq_scored_nominated_hand_kats.json come as objects too.  The CPU tests assert that the very set the GPU tests run meets every
hazard of the model."""
import json
import os

import numpy as np

import naive_ref as nv
import seq_nominated_ref as snr
import seq_nominated_scenes as sns
import seq_scored_ref as ssr
import seq_scored_scenes as sss

GI = sss.GI
I64_MAX = sss.I64_MAX
EDGE_N = [1, 63, 64, 65, 130, 8 * 64 - 1, 8 * 64, 8 * 64 + 1]
ROWS = (1, 7, 64, 300)
LANES = (0, 1, 4)
# the GPU parity set: (seed, nodes, rows, scalar lanes); every (nodes, lanes) pair once, the row counts rotating against both
PARITY = [(9400 + i, EDGE_N[i % 8], ROWS[(i + i // 8) % 4], LANES[i % 3]) for i in range(24)]
# ... and the kernel's lean form (more than four scalar lanes), with rows that carry those lanes
LEAN = [(9430, 130, 64, 5), (9431, 65, 7, 9), (9432, 8 * 64 + 1, 300, 12)]
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_scored_nominated_hand_kats.json")


def weights_of(seed):
    return sss.WEIGHTS[seed % len(sss.WEIGHTS)]


def make(seed, n_nodes, m, S, weights=None, n_pods=None, first_open=0, scalar_rows=False):
    """-> seq_nominated_scenes.make's dict plus weights.  scalar_rows: every row asks for most of what its node has left of one scalar, so
    that the row's scalar lane — or the key it brings — decides"""
    weights = weights_of(seed) if weights is None else weights
    rng = np.random.default_rng(seed ^ 0x5B)
    scn = sns.make(seed, n_nodes=n_nodes, m=m, n_groups=8, n_pods=min(200, 60 + 2 * n_nodes) if n_pods is None else n_pods, first_open=first_open,
                   n_scalars=S, names=sss.NAMES12 if S > 2 else None)
    sc, names = scn["sc"], scn["names"]
    templates = [dict(t) for t in {repr(sorted(p.requests.items())): p.requests for p in sc["pods"]}.values()]
    if seed % 2:                                                # seq_scored_scenes.make's spice, restated on this scene
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
                info.requested.MilliCPU = info.allocatable.MilliCPU - int(rng.integers(1, 4)) * t.get("cpu", 0)
    scored = ssr.replay(sc, weights, scalar_names=names)        # the table-less scored pass: its front is where the rows go
    front = sorted({k for k in scored["assumed"] if k >= 0}) or list(range(min(4, n_nodes)))
    own_rows = {int(r): i for i, r in enumerate(scn["own_id"]) if r != snr.NOM_NONE}
    for o in scn["nominees"]:
        if o.id in own_rows:
            at = scored["assumed"][own_rows[o.id]]
            if at >= 0 and rng.random() < 0.5:
                o.node = int(at)
            continue
        if o.req.MilliCPU >= (1 << 62) or rng.random() < 0.25:  # (the rows whose sums wrap, and a quarter of the others, stay where they are)
            continue
        o.node = int(rng.choice(front))
        info = sc["nodes"][o.node]
        free = max(min(info.allocatable.MilliCPU, 1 << 40) - max(info.requested.MilliCPU, 0), 0)
        o.req.MilliCPU = int(free * (rng.uniform(0.02, 0.3) if rng.random() < 0.5 else rng.uniform(0.3, 1.0)))
        if scalar_rows and names:
            nm = names[int(rng.integers(0, len(names)))]
            left = info.allocatable.ScalarResources.get(nm, 0) - (info.requested.ScalarResources or {}).get(nm, 0) if info.allocatable.ScalarResources else 0
            o.req.MilliCPU = 0
            o.req.ScalarResources = {nm: max(int(left) - int(rng.integers(0, 3)), 1)}
    others = [o for o in scn["nominees"] if o.id not in own_rows and o.req.MilliCPU < (1 << 62)]
    if seed % 4 == 1 and len(others) >= 3:                      # rows that make a tile wild: a negative lane, 2^40 and beyond
        others[0].req.MilliCPU, others[0].node = -int(rng.integers(100, 2000)), int(front[0])
        others[1].req.Memory, others[1].node = 1 << 40, int(front[len(front) // 2])
        others[2].req.MilliCPU, others[2].node = I64_MAX, int(front[-1])
    scn["weights"] = tuple(weights)
    return scn


def parity_scene(seed, n, m, S):
    return make(seed, n, m, S)


def lean_scene(seed, n, m, S):
    return make(seed, n, m, S, scalar_rows=True)


to_soa = sns.to_soa


def model(scn, weights=None):
    import seq_scored_nominated_ref as spr
    return spr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], scn["weights"] if weights is None else weights, scalar_names=scn["names"])


# ---- scenes built node by node --------------------------------------------------------------------------------------------------------------
def border_scene(n, weights):
    """N = 65 or 513: the last node of a tile of 64 and the first of the next are the two emptiest nodes, equal, each with a row that blocks
    the pods of priority <= 10 on it; the odd pods (priority 20) see neither row.  The node in front of them is the fullest that still holds a
    pod, with a row of its own (what the most-requested weights go for).  Every weight triple has to find its winners around the border."""
    b = n - 1                                                   # the first node of the last tile
    nodes = [sss._node(4000, 8 * GI, 1000 + 100 * (k % 7), (1 + k % 3) * GI) for k in range(n)]
    nodes[b - 2] = sss._node(4000, 8 * GI, 3000, 6 * GI)
    nodes[b - 1] = sss._node(4000, 8 * GI, 0, 0)
    nodes[b] = sss._node(4000, 8 * GI, 0, 0)
    pods = [nv.Pod(f"uid{i}", None, {"cpu": 500, "memory": GI}) for i in range(10)]
    priority = np.array([20 if i & 1 else 5 for i in range(10)], np.int32)
    rows = [snr.Nominee(0, b - 1, 10, nv.Resource(3800, 0, 0, 1, None)), snr.Nominee(1, b, 10, nv.Resource(3000, 0, 0, 1, None)),
            snr.Nominee(2, b - 2, 10, nv.Resource(600, 0, 0, 1, None))]
    sc = dict(nodes=nodes, cache={}, pods=pods, names=[], n_classes=1, denied=set(), permitted=set())
    return dict(sc=sc, names=[], priority=priority, own_id=np.full(10, snr.NOM_NONE, np.uint32), nominees=rows, rowless=None, weights=tuple(weights))


def walks_scene():
    """seq_scored_scenes.geometry_walks (N = 32 768 + 70: nodes 32 767 and 32 768 tie across the two tile walks) with a row on 32 767 that
    blocks the first pods' priority and not the last pod's: the tie goes to 32 768 first and to 32 767 later"""
    sc = sss.geometry_walks()
    priority = np.array([5, 5, 5, 5, 5, 20], np.int32)
    rows = [snr.Nominee(0, sss.WALK - 1, 10, nv.Resource(3500, 0, 0, 1, None))]
    return dict(sc=sc, names=[], priority=priority, own_id=np.full(6, snr.NOM_NONE, np.uint32), nominees=rows, rowless=None, weights=(1, 0, 1))


def waves_scene():
    """seq_scored_scenes.geometry_waves with a row on the better of the two nodes one lane of wave 1 sees (lane 5 of tile 65)"""
    sc = sss.geometry_waves()
    priority = np.array([5, 5, 20, 5, 20, 5], np.int32)
    rows = [snr.Nominee(0, 65 * 64 + 5, 10, nv.Resource(3200, 0, 0, 1, None))]
    return dict(sc=sc, names=[], priority=priority, own_id=np.full(6, snr.NOM_NONE, np.uint32), nominees=rows, rowless=None, weights=(1, 0, 1))


# ---- the hand-derived scenes ---------------------------------------------------------------------------------------------------------------
def load_kats():
    return json.load(open(KATS))["scenes"]


def kat_scene(k: dict, names=None):
    """one scene of the golden file as objects: seq_nominated_scenes.kat_scene's format plus `weights`"""
    scn = sns.kat_scene(k, names)
    scn["weights"] = tuple(k["weights"])
    return scn
