"""The hand known answers of bs_preempt_commit (tests/golden/preempt_commit_hand_kats.json) as soa objects, for the CPU and GPU tests."""
from __future__ import annotations

import json
import os

from preempt_scenes import kat_scene

HERE = os.path.dirname(os.path.abspath(__file__))


def commit_kats():
    with open(os.path.join(HERE, "golden", "preempt_commit_hand_kats.json")) as f:
        return json.load(f)["scenes"]


def kat_commit_scene(sc: dict) -> dict:
    s = kat_scene(sc)
    s.update(cap=sc["cap"], apply=sc["flags"]["apply"], assume=sc["flags"]["assume"])
    return s
