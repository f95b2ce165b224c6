"""Scenes for the two sampled passes (TEST INFRASTRUCTURE), for tests/test_seq_sampled_cpu.py and tests/test_gpu_seq_sampled.py: the grid of
list lengths, cursors and sample sizes around the kernel's geometry (a slot is 64 nodes, a round 8 slots = 512 nodes), seeded scenes built
with seq_scored_scenes.make (rule P underneath) and seq_scored_nominated_scenes.make (rule SP underneath), and scenes built node by node:
a candidate set of known size, tiles the first-fit bounds exclude, and the hand-derived scenes of tests/golden/seq_sampled_hand_kats.json.
A CASE is a hashable tuple; `scene`, `to_soa` and `model` turn it into objects, arrays and the object model's answer.  The CPU tests assert
that the very cases the GPU tests run meet every hazard of the model."""
import functools
import json
import os

import numpy as np

import naive_ref as nv
import seq_nominated_ref as snr
import seq_nominated_scenes as sns
import seq_sampled_ref as smr
import seq_scored_nominated_scenes as sps
import seq_scored_scenes as sss

GI = sss.GI
GRID_N = [1, 63, 64, 65, 128, 129, 511, 512, 513, 1025]        # one round of the walk covers 512 nodes
LANES = (0, 1, 4)
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_sampled_hand_kats.json")


def starts(n):
    """the cursors of the grid: distinct values of 0, 1, 63, 64, N - 1, N, N + 7 (the pass takes them mod N)"""
    out = []
    for s in (0, 1, 63, 64, n - 1, n, n + 7):
        if s not in out:
            out.append(s)
    return out


def sizes(n):
    return [1, 2, 64, 0, n, n + 1]


def grid_pods(n):
    return 40 if n <= 129 else 24


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
# ("grid", form, N index, start, K, weights): form "P" or "SP"
def _grid_p():
    out = []
    for ni, n in enumerate(GRID_N):
        for si, s in enumerate(starts(n)):
            for ki, k in enumerate(sizes(n)):
                w = (0, 0, 0) if (si + ki) % 6 == 5 else sss.WEIGHTS[(ni + si + ki) % len(sss.WEIGHTS)]
                out.append(("grid", "P", ni, s, k, w))
    return out


def _grid_sp():
    """under rule SP every N meets every cursor and every sample size once (a diagonal of the plain form's grid)"""
    out = []
    for ni, n in enumerate(GRID_N):
        ss, ks = starts(n), sizes(n)
        for j in range(max(len(ss), len(ks))):
            w = (0, 0, 0) if j == 5 else sss.WEIGHTS[(ni + j) % len(sss.WEIGHTS)]
            out.append(("grid", "SP", ni, ss[j % len(ss)], ks[(j + ni) % len(ks)], w))
    return out


GRID_P, GRID_SP = _grid_p(), _grid_sp()
# the lane counts of one N, both forms: 5, 9 and 12 take the kernel's lean form
LANE_CASES = [("lanes", form, S, 77, 3, (1, 0, 1)) for form in ("P", "SP") for S in (0, 1, 4, 5, 9, 12)]
KNOWN_C = 12                                                     # |C| of every pod of known_scene
KNOWN_CASES = [("known", "P", 150, KNOWN_C + d, (3, 2, 1)) for d in (-1, 0, 1)]
PRUNE_CASE = ("prune", "P", 200, 5, (1, 0, 1))
PRUNE_CASE_1 = ("prune", "P", 70, 5, (1, 0, 1))                 # the same scene from a cursor inside the other excluded tile
FAR_CASES = [("far", "P", 8, k, (1, 0, 1)) for k in (1, 2, 4, 5)]
FILTER_SEEDS = list(range(9100, 9110))
F1_CASES = [("grid", "P", 4, 0, 0, (1, 0, 1)), ("grid", "P", 8, 0, 513, (3, 2, 1)), ("lanes", "P", 9, 0, 0, (1, 0, 1)),
            ("grid", "SP", 4, 0, 0, (1, 0, 1)), ("grid", "SP", 8, 0, 514, (3, 2, 1)), ("lanes", "SP", 12, 0, 0, (0, 1, 0))]
CHAIN_CASE = ("grid", "P", 5, 100, 3, (1, 0, 1))                # 129 nodes, gangs


def filter_case(seed, start, k):
    return ("filter", "P", seed, start, k, (1, 0, 1))


FILTER_CASE = filter_case(9105, 7, 3)


def all_gpu_cases():
    """every case whose model the GPU tests compare a pass with (the F1 twins and the hand-derived scenes are held by their own tests)"""
    return GRID_P + GRID_SP + LANE_CASES + KNOWN_CASES + FAR_CASES + [PRUNE_CASE, PRUNE_CASE_1, FILTER_CASE, CHAIN_CASE]


# ---- scenes built node by node -------------------------------------------------------------------------------------------------------------------
def known_scene():
    """200 nodes, ten ungrouped pods of 500 mCPU / 1 GiB.  Every node is full except twelve roomy ones (room for all ten pods on each), so
    |C| = 12 for every pod: K = 11 stops at the twelfth member, K = 12 is |C| exactly (no stop, V = N), K = 13 is more than there is."""
    nodes = [sss._node(4000, 8 * GI, 4000, 0) for _ in range(200)]
    for j, k in enumerate((3, 40, 63, 64, 65, 100, 127, 128, 149, 150, 190, 199)):
        nodes[k] = sss._node(64000, 128 * GI, 1000 * (j % 5), (j % 3) * GI)
    return sss._scene(nodes, [nv.Pod(f"uid{i}", None, {"cpu": 500, "memory": GI}) for i in range(10)])


PRUNE_N = 6 * 64 + 10
PRUNE_OPEN = (3, 10, 130, 140, 260, 330, 390)


def prune_scene():
    """394 nodes in seven tiles, four ungrouped pods of 1000 mCPU / 1 GiB.  Every node is full except seven: tiles 1 and 3 hold none, so
    the first-fit bounds exclude them.  The first walk starts at 200, inside excluded tile 3; its members in visit order are 260, 330, 390,
    then behind the wrap 3 and 10 (the fifth: K = 5), then — across excluded tile 1 — 130, which ends the walk: V = 130 + 394 - 200 = 324."""
    nodes = [sss._node(4000, 8 * GI, 4000, 0) for _ in range(PRUNE_N)]
    for j, k in enumerate(PRUNE_OPEN):
        nodes[k] = sss._node(8000, 16 * GI, 500 * j, 0)
    return sss._scene(nodes, [nv.Pod(f"uid{i}", None, {"cpu": 1000, "memory": GI}) for i in range(4)])


FAR_N = 1025
FAR_OPEN = (2, 10, 520, 530, 1000, 1024)


def far_scene():
    """1025 nodes in seventeen tiles — three rounds of the walk, the last tile holds one node —, three ungrouped pods.  Every node is full
    except six.  From the cursor 8 the members come at visit positions 2 (node 10, round 0), 512 and 522 (nodes 520 and 530: one slot of
    round 1), 992 (node 1000), 1016 (node 1024, round 2) and, behind the wrap, 1019 (node 2: the low lanes of the cursor's tile).  K = 1
    ends the walk in round 1 on a member whose predecessor sits in round 0; K = 5 ends it in the revisited lanes."""
    nodes = [sss._node(4000, 8 * GI, 4000, 0) for _ in range(FAR_N)]
    for j, k in enumerate(FAR_OPEN):
        nodes[k] = sss._node(8000, 16 * GI, 500 * j, 0)
    return sss._scene(nodes, [nv.Pod(f"uid{i}", None, {"cpu": 1000, "memory": GI}) for i in range(3)])


# ---- case -> scene, arrays, model -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scn(kind, form, which):
    """the scene of a case without its sample and weights: a dict in seq_scored_nominated_scenes.make's format (nominees None under rule P)"""
    if kind == "grid":
        n = GRID_N[which]
        if form == "P":
            sc = sss.make(9500 + which, n_nodes=n, n_groups=6, n_pods=grid_pods(n), n_scalars=LANES[which % 3], gangs=which % 4 != 3)
            return dict(sc=sc, names=sc["names"], nominees=None, priority=None, own_id=None)
        return sps.make(9540 + which, n, (1, 7, 64, 300)[which % 4], LANES[which % 3], weights=(1, 0, 1), n_pods=grid_pods(n))
    if kind == "lanes":
        if form == "P":
            sc = sss.make(9560 + which, n_nodes=130, n_groups=6, n_pods=60, n_scalars=which)
            return dict(sc=sc, names=sc["names"], nominees=None, priority=None, own_id=None)
        return sps.make(9580 + which, 130, 64, which, weights=(1, 0, 1), n_pods=60, scalar_rows=which > 4)
    if kind == "filter":
        sc = sss.filter_scene(which)
        return dict(sc=sc, names=sc["names"], nominees=None, priority=None, own_id=None)
    if kind == "kat":
        k = load_kats()[which]
        scn = sns.kat_scene(dict(k, rows=k.get("rows", [])))
        if k["form"] == "P":
            scn["nominees"] = None
        return scn
    sc = dict(known=known_scene, prune=prune_scene, far=far_scene)[kind]()
    return dict(sc=sc, names=sc["names"], nominees=None, priority=None, own_id=None)


def split(case):
    """-> (scene key, sample (num_to_find, start), weights, stages has Filter)"""
    kind, form = case[0], case[1]
    if kind in ("grid", "lanes", "filter"):
        return (kind, form, case[2]), (case[4], case[3]), case[5], kind == "filter"
    if kind == "kat":
        k = load_kats()[case[2]]
        return (kind, k["form"], case[2]), tuple(k["sample"]), tuple(k["weights"]), False
    return (kind, form, 0), (case[3], case[2]), case[4], False


def scene(case):
    return _scn(*split(case)[0])


@functools.lru_cache(maxsize=None)
def to_soa(key):
    """(nodes, fit, groups, pods, owner_ids, rows or None) of a scene key (split(case)[0]): what the device is loaded with"""
    scn = _scn(*key)
    if scn["nominees"] is None:
        return sss.to_soa(scn["sc"]) + (None,)
    return sns.to_soa(scn)


@functools.lru_cache(maxsize=None)
def model(case):
    key, sample, weights, flt = split(case)
    scn = _scn(*key)
    return smr.replay(scn["sc"], weights, sample, run_filter=flt, scalar_names=scn["names"], nominees=scn["nominees"], priority=scn["priority"],
                      own_id=scn["own_id"])


# ---- the hand-derived file ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def load_kats():
    return json.load(open(KATS))["scenes"]
