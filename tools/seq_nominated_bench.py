"""bs_seq_run_nominated timed beside bs_seq_run on a synthetic configuration, one context, one process: (1) bs_seq_run; (2) the nominated
form with an empty table and no own ids; (3) with `--rows` rows (default 4096) on the first-fit front — the nodes the row-less pass fills
first —, priorities drawn around the queue's; (4) the same with BS_SEQ_NO_CURSOR=1.  Every repetition reloads nodes, groups, pods and the
table, so every pass starts from the same state; one untimed pass of each form first, so that no figure contains a code-object load.  The
figures are the wall time of the call as the caller sees it (the calls are synchronous) and the kernel's own clock (total_ns), best and
median of `--reps` runs (default 5), and each form's spread (max - min) so that a ratio can be read against the noise of the same run.
Prints one JSON line.  Usage: python tools/seq_nominated_bench.py [config] [scenario] [--reps N] [--rows M]"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bsa = importlib.import_module("batch-scheduler_amd")
soa = bsa.soa


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.isdigit()]
    config = args[0] if args else "cfg3"
    scenario = args[1] if len(args) > 1 else "tail"
    reps, m = opt("--reps", 5), opt("--rows", 4096)
    nodes, fit, groups, pods, _ = bsa.synth.make(config, scenario)
    pods = pods.take(np.argsort(pods.group, kind="stable"))           # Compare order
    rng = np.random.default_rng(17)
    prio = rng.integers(0, 4, size=pods.p).astype(np.int32) * 10
    out = {"config": f"{config}/{scenario}", "pods": int(pods.p), "nodes": int(nodes.n), "groups": int(groups.g), "reps": reps, "rows": m, "forms": {}}
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:
        def load(table):
            ctx.load_nodes(nodes, fit)
            ctx.load_groups(groups)
            ctx.load_pods(pods)
            if table is not None:
                ctx.nominated_load(*table)

        load(None)
        first = ctx.seq_run(soa.STAGE_PREFILTER)
        wait = ctx.seq_waiting_read()
        used = np.unique(np.concatenate([first["pod_node"][first["pod_node"] >= 0], wait[wait >= 0]]))
        front = used if used.size else np.arange(min(nodes.n, 64))
        node = front[rng.integers(0, front.size, size=m)].astype(np.uint32)
        free = np.maximum(nodes.allocatable[0] - nodes.requested[0], 0)[node]
        req = np.zeros((nodes.lanes, m), np.int64)
        req[0] = (free * rng.uniform(0.05, 0.5, size=m)).astype(np.int64)
        table = (node, (rng.integers(0, 4, size=m) * 10 + rng.integers(-1, 2, size=m)).astype(np.int32), req, np.zeros(m, np.uint32))
        empty = (np.zeros(0, np.uint32), np.zeros(0, np.int32), np.zeros((nodes.lanes, 0), np.int64), np.zeros(0, np.uint32))
        forms = (("seq_run", None, None), ("nominated_empty", empty, None), ("nominated_rows", table, None), ("nominated_rows_no_cursor", table, "1"))
        for name, tab, nocur in forms:
            if nocur:
                os.environ["BS_SEQ_NO_CURSOR"] = nocur
            wall, dev, placed = [], [], 0
            for rep in range(reps + 1):                                # (the first one is the warm-up)
                load(tab)
                t = time.perf_counter()
                r = ctx.seq_run(soa.STAGE_PREFILTER) if tab is None else ctx.seq_run_nominated(prio, None)
                dt = time.perf_counter() - t
                if rep:
                    wall.append(dt)
                    dev.append(r["total_ns"])
                placed = int((r["pod_node"] >= 0).sum())
            os.environ.pop("BS_SEQ_NO_CURSOR", None)
            out["forms"][name] = {"wall_ms_best": min(wall) * 1e3, "wall_ms_median": float(np.median(wall)) * 1e3, "wall_ms_spread": (max(wall) - min(wall)) * 1e3,
                                  "kernel_ms_best": min(dev) / 1e6, "kernel_ms_median": float(np.median(dev)) / 1e6, "kernel_ms_spread": (max(dev) - min(dev)) / 1e6,
                                  "pods_released": placed, "node_picks": r["node_picks"], "pick_rounds": r["pick_rounds"]}
        base = out["forms"]["seq_run"]["kernel_ms_median"]
        out["ratio_to_seq_run_kernel_median"] = {k: v["kernel_ms_median"] / base for k, v in out["forms"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
