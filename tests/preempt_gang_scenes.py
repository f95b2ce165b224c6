"""Scenes of bs_preempt_commit_gang for the CPU and GPU tests: the hand known answers (tests/golden/preempt_gang_hand_kats.json) as soa
objects with their check, and seeded random scenes whose preemptor lists are cut into gangs (one priority a gang, one run each) with
needs drawn so that runs stand and runs miss."""
from __future__ import annotations

import json
import os

import numpy as np

import preempt_gang_ref as gr
import preempt_pdb_ref as pp
from preempt_commit_scenes import kat_commit_scene

HERE = os.path.dirname(os.path.abspath(__file__))
STATE = ("req", "pres", "bound_id", "bound_node")


def gang_kats():
    with open(os.path.join(HERE, "golden", "preempt_gang_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_gang_scene(sc: dict) -> dict:
    s = kat_commit_scene(sc)
    s["need"] = np.array(sc["need"], np.uint32)
    return s


def check_gang_kat(got: dict, sc: dict, where: str):
    """got: res (with n_pdb_violations), req, pres, bound_id, bound_node, slot_voided, group_placed against the hand-derived scene"""
    pp.check_pdb_kat(got, sc, where)
    st = sc["expect_state"]
    assert np.array_equal(np.asarray(got["req"]), np.array(st["req"], np.int64)), f"{where}: node requests {np.asarray(got['req']).tolist()}"
    assert np.array_equal(np.asarray(got["pres"]), np.array(st["pres"], np.uint32)), f"{where}: present bits"
    assert list(got["bound_id"]) == st["bound_id"] and list(got["bound_node"]) == st["bound_node"], f"{where}: bound table {list(got['bound_id'])}"
    assert list(got["slot_voided"]) == sc["slot_voided"], f"{where}: slot_voided {list(got['slot_voided'])}"
    assert list(got["group_placed"]) == sc["group_placed"], f"{where}: group_placed {list(got['group_placed'])}"


def gang_scene(seed: int, n: int, per_node, S: int, q: int, groups: int = 9, share: float = 0.0, need_share: float = 0.8, **kw) -> dict:
    """preempt_pdb_ref.pdb_scene (distinct preemptors, requests that need several victims) whose grouped preemptors get their gang's
    priority, listed in gang_order (one run a gang); sc["need"][g] is drawn between 1 and the gang's member count + 1 for need_share of
    the gangs in the list, 0 for the others; sc["violating"] are the PDB bits (share of the bound pods)."""
    sc, bits = pp.pdb_scene(seed, n=n, per_node=per_node, S=S, q=q, groups=groups, share=share, **kw)
    rng = np.random.default_rng(seed ^ 0x6A46)
    grp = np.asarray(sc["pods"].group)[sc["pod_index"]].astype(np.int64)
    prio = sc["priority"].astype(np.int64).copy()
    need = np.zeros(sc["groups"], np.uint32)
    for g in np.unique(grp[grp >= 0]):
        m = grp == g
        prio[m] = prio[m][0]
        if rng.random() < need_share:
            # small needs stand often, needs near the member count miss often
            need[g] = rng.integers(1, int(m.sum()) + 2) if rng.random() < 0.5 else rng.integers(1, 3)
    o = gr.gang_order(grp, prio)
    sc["pod_index"], sc["priority"] = sc["pod_index"][o], prio[o].astype(np.int32)
    sc["need"], sc["violating"] = need, bits
    return sc


def expect(sc: dict, cap: int, apply=False, assume=False) -> dict:
    """the numpy restatement (the defining property) of the scene"""
    prep = pp.PdbPrep(sc["nodes"], sc["bound"], sc["S"], sc.get("violating"))
    return gr.gang_np(prep, sc["fit"], sc["pods"], sc["bound"], sc["pod_index"], sc["priority"], sc["protected"], sc["need"], cap, apply, assume)


def expect_obj(sc: dict, cap: int, apply=False, assume=False) -> dict:
    return gr.gang_obj(sc["nodes"], sc["fit"], sc["pods"], sc["bound"], sc["S"], sc["pod_index"], sc["priority"], sc["protected"], sc["need"],
                       cap, apply, assume, sc.get("violating"))
