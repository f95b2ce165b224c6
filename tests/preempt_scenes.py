"""Preemption scenes shared by the CPU and GPU tests: the hand known answers (tests/golden/preempt_hand_kats.json) as soa objects, and
random scenes from synth.make_bound / make_preemptors."""
from __future__ import annotations

import importlib
import json
import os

import numpy as np

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth = bsa.soa, bsa.synth
HERE = os.path.dirname(os.path.abspath(__file__))


def hand_kats():
    with open(os.path.join(HERE, "golden", "preempt_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_scene(sc: dict) -> dict:
    nd, pd, bd = sc["nodes"], sc["pods"], sc["bound"]
    nodes = soa.Nodes(np.array(nd["alloc"], np.int64), np.array(nd["req"], np.int64), nd["apres"], nd["rpres"], nd["flags"])
    fit = soa.FitMasks.from_bool(np.array(sc["fit"], bool))
    p = len(pd["group"])
    pods = soa.Pods(pd["group"], np.array(pd["req"], np.int64), pd["pres"], pd["cls"], np.zeros(p, np.uint64), np.zeros(p, np.uint8))
    bound = soa.Bound(bd["node"], bd["priority"], bd["start_ns"], bd["group"], np.array(bd["req"], np.int64).reshape(4 + sc["S"], -1),
                      bd["req_present"])
    pre = sc["preemptors"]
    return dict(nodes=nodes, fit=fit, pods=pods, bound=bound, S=sc["S"], protected=np.array(sc["protected"], np.uint8),
                pod_index=np.array(pre["pod_index"], np.uint32), priority=np.array(pre["priority"], np.int32), groups=len(sc["protected"]))


def random_scene(seed: int, n: int, per_node, S: int, q: int, groups: int = 6, p: int = 40, classes: int = 3, fit_density: float = 0.8,
                 protected_share: float = 0.3, levels=synth.PRIORITY_LEVELS, flagged: float = 0.05) -> dict:
    bound, nodes = synth.make_bound(seed, n, groups, per_node, S, flagged=flagged, levels=levels)
    fitb = synth.Stream(seed ^ 0xF17, 1).uniform(classes * n).reshape(classes, n) < fit_density
    pods, pod_index, priority = synth.make_preemptors(seed, q, p, groups, S, classes, levels=levels)
    protected = (synth.Stream(seed ^ 0xF17, 2).uniform(groups) < protected_share).astype(np.uint8)
    return dict(nodes=nodes, fit=soa.FitMasks.from_bool(fitb), pods=pods, bound=bound, S=S, protected=protected, pod_index=pod_index,
                priority=priority, groups=groups)


def groups_for(sc: dict) -> "soa.Groups":
    """a group state of the scene's group count (bs_preempt_run reads nothing of it but g)"""
    g = soa.Groups.empty(sc["groups"], 4 + sc["S"])
    g.min_member[:] = 1
    return g


def ungrouped_scene(sc: dict) -> dict:
    """the scene for a context that holds no groups: every queue pod and every bound pod ungrouped, an empty protected list, and a group
    state of zero groups from groups_for"""
    sc["bound"].group[:] = soa.POD_NOT_GROUPED
    sc["pods"].group[:] = soa.POD_NOT_GROUPED
    sc["protected"] = np.zeros(0, np.uint8)
    sc["groups"] = 0
    return sc
