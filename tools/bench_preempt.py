"""Times bs_preempt_run (the batched gang-aware victim search, csrc/bs_preempt.hpp) at the cfg3 and cfg4 node counts with 20-110 bound
pods per node, for 64 and 1024 preemptors.  Prints one JSON line: ms per call (median of --reps calls after --warmup), end to end
through the C ABI (upload of the preemptor arrays, both launches, the result copy)."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bsa = importlib.import_module("batch-scheduler_amd")
soa, synth = bsa.soa, bsa.synth


def one(config: str, q: int, reps: int, warmup: int) -> dict:
    cfg = synth.CONFIGS[config]
    n, S = cfg["nodes"], cfg["scalars"]
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    pods, pidx, prio = synth.make_preemptors(20260921, q, 4096, cfg["groups"], S, cfg["classes"])
    groups = soa.Groups.empty(cfg["groups"], 4 + S)
    prot = (synth.Stream(20260921, 99).uniform(cfg["groups"]) < 0.3).astype(np.uint8)
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        ctx.load_bound(bound)
        for _ in range(warmup):
            r = ctx.preempt(pidx, prio, prot, victim_cap=16)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = ctx.preempt(pidx, prio, prot, victim_cap=16)
            ts.append((time.perf_counter() - t0) * 1e3)
    return dict(config=config, nodes=n, bound=int(bound.b), preemptors=q, ms=round(float(np.median(ts)), 4), ms_min=round(float(min(ts)), 4),
                placed=int((r["node"] >= 0).sum()), with_victims=int((r["n_victims"] > 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rows = [one(c, q, a.reps, a.warmup) for c in ("cfg3", "cfg4") for q in (64, 1024)]
    print(json.dumps(dict(metric="bs_preempt_run ms per call", rows=rows)))


if __name__ == "__main__":
    main()
