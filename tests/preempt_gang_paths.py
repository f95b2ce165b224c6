"""Which paths k_gang_resolve's quorum and rollback (csrc/bs_preempt_commit_gang.hpp) have to take for a scene, established on the
object-level restatement (tests/preempt_gang_ref.py, gang_obj: its trace holds what every run's slots answered BEFORE the decision), in
the style of tests/preempt_commit_paths.py.  A GPU test asserts the path it is about before it trusts its comparison.

classify(sc, cap) -> dict of counts:
  voided_placed      voided runs with at least one slot that had a node (a rollback with work to do)
  voided_empty       voided runs none of whose slots had a node
  standing           runs that met their need
  same_node          voided runs two of whose slots chose the same node (bit words restored last slot first, two nominees in dn)
  revictim           bound pods evicted by a voided run and evicted again by a later slot that stands
  dirty_reuse        later standing slots that chose a node a voided run had touched (a dirty node with zero deltas)
  over_cap           voided slots with more victims than victim_cap (the undo cannot read the truncated row)
  big_voided         voided slots with three or more victims
  pdb_voided         voided slots whose answer had PDB violations;  pdb_standing: standing slots with violations
  run_at_end         the slot list ends with a run;  back_to_back: two runs next to each other at one priority;  run_of_one
  need_eq_placed     standing runs with placed == need;  need_gt_len: runs whose need exceeds their length
  ungrouped_between  slots outside every run that lie between two runs"""
from __future__ import annotations

import numpy as np

import preempt_commit_ref as pc
import preempt_gang_scenes as gs


def classify(sc: dict, cap: int) -> dict:
    got = gs.expect_obj(sc, cap)
    tr, ans = got["trace"], got["answered"]
    order = [int(i) for i in pc.slot_order(sc["priority"])]
    slot_of = {i: s for s, i in enumerate(order)}
    in_voided = {sl["preemptor"] for r in tr if r["voided"] for sl in r["slots"]}
    c = dict.fromkeys(("voided_placed", "voided_empty", "standing", "same_node", "revictim", "dirty_reuse", "over_cap", "big_voided", "pdb_voided", "pdb_standing",
                       "run_at_end", "back_to_back", "run_of_one", "need_eq_placed", "need_gt_len", "ungrouped_between"), 0)
    for x, r in enumerate(tr):
        length = r["last"] - r["first"] + 1
        c["run_of_one"] += length == 1
        c["need_gt_len"] += r["need"] > length
        c["run_at_end"] += r["last"] == len(order) - 1
        if x and tr[x - 1]["last"] + 1 == r["first"] and sc["priority"][order[r["first"]]] == sc["priority"][order[tr[x - 1]["last"]]]:
            c["back_to_back"] += 1
        if x and tr[x - 1]["last"] + 1 < r["first"]:
            c["ungrouped_between"] += r["first"] - tr[x - 1]["last"] - 1
        if not r["voided"]:
            c["standing"] += 1
            c["need_eq_placed"] += r["placed"] == r["need"]
            continue
        c["voided_placed" if r["placed"] else "voided_empty"] += 1
        nodes = [sl["node"] for sl in r["slots"] if sl["node"] >= 0]
        c["same_node"] += len(nodes) != len(set(nodes))
        vics = {v for sl in r["slots"] for v in sl["victims"]}
        c["over_cap"] += sum(len(sl["victims"]) > cap for sl in r["slots"])
        c["big_voided"] += sum(len(sl["victims"]) >= 3 for sl in r["slots"])
        c["pdb_voided"] += sum(sl["n_pdb_violations"] > 0 for sl in r["slots"])
        for i, a in ans.items():
            if i in in_voided or slot_of[i] <= r["last"] or a["node"] < 0:
                continue
            c["revictim"] += len(vics & set(a["victims"]))
            c["dirty_reuse"] += a["node"] in nodes
    c["pdb_standing"] = sum(a["n_pdb_violations"] > 0 for i, a in ans.items() if i not in in_voided)
    return {k: int(v) for k, v in c.items()}


def summary(c: dict) -> str:
    return " ".join(f"{k}={v}" for k, v in c.items() if v)
