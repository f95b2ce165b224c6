"""bs_bound_bind timed on a cfg3-sized state after a pass: one released gang bound, 32 released gangs bound, and every gang the pass released
bound, beside what the call replaces — bs_wait_release of the gangs, the pass's pod_node, the rows' columns marshalled on the host
(vectorised numpy over the caller's own copy of the queue) and bs_bound_apply.  Both are timed in the same process on a freshly prepared
context each (nodes, groups, queue and bound table loaded, the pass run, the empty wait table loaded), after one untimed bind of each kind
so that no figure contains a code-object load.  Every figure is the wall time of the call(s) as the caller sees them; best and median of
`--reps` runs (at least 20).  No threshold is set.  Usage: python tools/bind_bench.py [config] [scenario] [--reps N] [--per-node N]"""
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


def fresh(ctx, nodes, fit, groups, pods, bound):
    """-> the pass's result"""
    ctx.load_nodes(nodes, fit)
    ctx.load_groups(groups)
    ctx.load_pods(pods)
    ctx.load_bound(bound)
    r = ctx.seq_run(soa.STAGE_PREFILTER)
    ctx.wait_load()
    return r


def new_way(ctx, pl, prio, start):
    t = time.perf_counter()
    ctx.bound_bind((), pl, prio, start)
    return time.perf_counter() - t


def old_way(ctx, gangs, pl, pod_node, pods, prio, start):
    """bs_wait_release (the gangs' rows of earlier cycles: none on this state, the call is still made), pod_node, the columns from the
    caller's copy of the queue, bs_bound_apply"""
    t = time.perf_counter()
    rel = ctx.wait_release(gangs)
    assert rel["n"] == 0
    ins = soa.Bound(pod_node[pl].astype(np.uint32), prio, start, pods.group[pl], np.ascontiguousarray(pods.req[:, pl]), pods.req_present[pl])
    ctx.bound_apply(None, ins)
    return time.perf_counter() - t


def main():
    opts = ("--reps", "--per-node")
    opt = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default      # noqa: E731
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in opts]
    config = args[0] if args else "cfg3"
    scenario = args[1] if len(args) > 1 else "tail"
    reps = max(opt("--reps", 21), 20)
    nodes, fit, groups, pods, _ = synth.make(config, scenario)
    pods = pods.take(np.argsort(pods.group, kind="stable"))           # Compare order
    S = nodes.lanes - 4
    bound, _ = synth.make_bound(7, nodes.n, groups.g, opt("--per-node", 20), S)
    rng = np.random.default_rng(3)
    out = {"config": f"{config}/{scenario}", "pods": int(pods.p), "nodes": int(nodes.n), "groups": int(groups.g), "bound": int(bound.b), "reps": reps, "modes": {}}
    with bsa.Context(scalar_lanes=S) as ctx:
        r = fresh(ctx, nodes, fit, groups, pods, bound)
        pod_node = r["pod_node"]
        released = r["released_group"].astype(np.uint32)
        placed = np.nonzero(pod_node >= 0)[0]
        out["released_gangs"], out["placed_pods"] = int(released.size), int(placed.size)
        if not released.size:
            print(json.dumps(out))
            return
        warm = placed[pods.group[placed] == released[0]]
        new_way(ctx, warm, np.zeros(warm.size, np.int32), np.zeros(warm.size, np.int64))
        fresh(ctx, nodes, fit, groups, pods, bound)
        old_way(ctx, released[:1], warm, pod_node, pods, np.zeros(warm.size, np.int32), np.zeros(warm.size, np.int64))
        for name, gangs in (("1_gang", released[:1]), ("32_gangs", released[:: max(released.size // 32, 1)][:32]), ("all_released", released)):
            pl = placed[np.isin(pods.group[placed], gangs)]
            prio, start = rng.integers(0, 5, pl.size).astype(np.int32), rng.integers(0, 1 << 40, pl.size).astype(np.int64)
            new, old = [], []
            for _ in range(reps):
                fresh(ctx, nodes, fit, groups, pods, bound)
                new.append(new_way(ctx, pl, prio, start))
                a = ctx.read_bound()
                fresh(ctx, nodes, fit, groups, pods, bound)
                old.append(old_way(ctx, gangs, pl, pod_node, pods, prio, start))
                b = ctx.read_bound()
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the two ways give the same table"
            out["modes"][name] = {"gangs": int(len(gangs)), "rows": int(pl.size),
                                  "bound_bind_us_best": min(new) * 1e6, "bound_bind_us_median": float(np.median(new)) * 1e6,
                                  "release_marshal_apply_us_best": min(old) * 1e6, "release_marshal_apply_us_median": float(np.median(old)) * 1e6}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
