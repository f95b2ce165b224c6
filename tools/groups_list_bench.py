"""bs_groups_list_apply timed on a cfg3-sized context (2k groups, 10k pods, 5k nodes) that holds the wait table of tools/wait_bench.py's scene
(the waiting pods of one pass, parked) and the bound-pod table of tools/bench_preempt.py's (synth.make_bound), for four deltas — one group
appended, one removed, 32 removed plus 32 appended, 1 % removed plus as many appended — beside the reload path the call replaces, in the same
process: bs_groups_load of the new list, the queue's group column remapped on the host (vectorised numpy) and bs_pods_load, bs_wait_read /
remap / bs_wait_load, the bound table's group column remapped and bs_bound_load, then the stream.  Both paths are also timed through to the
first bs_batch_map behind them (a latency-mode batch with every stage): what either path leaves to be re-derived is paid there.  The new group
list and the caller's own copies of the queue and the bound table are prepared outside the timed regions of both paths.  One untimed call
first, so that no figure contains the new kernels' code-object load.  Every figure is wall time as the caller sees it, best and median of
`--reps` runs, each on a freshly loaded context.  No threshold is set.  Usage: python tools/groups_list_bench.py [config] [scenario] [--reps N]"""
import ctypes as C
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
COLUMNS = ("min_member", "status_scheduled", "matched", "flags", "cls", "min_resources", "min_resources_present", "occupied_by")
STAGES = soa.STAGE_ALL | soa.BATCH_HOST_RESULTS


def fresh(ctx, nodes, fit, groups, pods, bound):
    ctx.load_nodes(nodes, fit)
    ctx.load_groups(groups)
    ctx.load_pods(pods)
    ctx.seq_run(soa.STAGE_PREFILTER)
    ctx.wait_load()
    ctx.wait_park(cap=0)
    ctx.load_bound(bound)
    ctx.run(STAGES)                                            # a cycle's batch has run: classes, pairs and directories are resident
    ctx.sync()


def first_batch(ctx):
    ctx.run(STAGES)
    try:
        ctx.map_results()
    except bsa.BsError as e:                                   # (no host results on this chain: the stream is waited for instead)
        if e.status != -4:
            raise
        ctx.sync()


def index_map(g, remove):
    rem = np.asarray(remove, np.int64)
    new = np.arange(g, dtype=np.int64) - np.searchsorted(rem, np.arange(g), side="left")
    new[rem] = -1
    return new.astype(np.int32)


def remap(col, imap):
    col = col.copy()
    inside = (col >= 0) & (col < imap.size)
    new = imap[col[inside]]
    col[inside] = np.where(new < 0, soa.POD_GROUP_MISSING, new)
    return col


def new_list(cur, remove, rows):
    keep = np.setdiff1d(np.arange(cur.g), remove)
    return soa.Groups(*[np.concatenate([getattr(cur, n)[..., keep], getattr(rows, n)], axis=-1) for n in COLUMNS])


def reload_path(ctx, new_groups, imap, pods, bound, sync):
    """the path the call replaces; -> seconds"""
    t = time.perf_counter()
    tab = ctx.wait_read()                                      # (before the new list: afterwards the table's group count is stale)
    ctx.load_groups(new_groups)
    q = pods.copy()
    q.group[:] = remap(pods.group, imap)
    ctx.load_pods(q)
    keep = imap[tab["group"]] >= 0
    ctx.wait_load(tab["node"][keep], imap[tab["group"][keep]], tab["req"][:, keep], tab["req_present"][keep])
    ctx.load_bound(soa.Bound(bound.node, bound.priority, bound.start_ns, remap(bound.group, imap), bound.req, bound.req_present))
    sync()
    return time.perf_counter() - t


def main():
    argv = sys.argv[1:]
    reps = 7
    if "--reps" in argv:
        at = argv.index("--reps")
        reps = int(argv[at + 1])
        del argv[at:at + 2]
    config = argv[0] if argv else "cfg3"
    scenario = argv[1] if len(argv) > 1 else "tail"
    nodes, fit, groups, pods, _ = synth.make(config, scenario)
    pods = pods.take(np.argsort(pods.group, kind="stable"))           # Compare order
    cfg = synth.CONFIGS[config]
    bound, _ = synth.make_bound(20260921, cfg["nodes"], cfg["groups"], (20, 110), cfg["scalars"])
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(11)
    g = groups.g
    out = {"config": f"{config}/{scenario}", "pods": int(pods.p), "nodes": int(nodes.n), "groups": int(g), "bound_entries": int(bound.b), "reps": reps, "modes": {}}
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:
        stream = C.c_void_p(ctx.stream())
        sync = lambda: hip.hipStreamSynchronize(stream)
        fresh(ctx, nodes, fit, groups, pods, bound)
        out["wait_rows"] = ctx.wait_count()
        ctx.groups_list_apply([1], [], soa.Groups.empty(0, nodes.lanes), wait_cap=0)      # warm-up: the first launch of the k_gl_* kernels loads their code
        one_percent = max(g // 100, 1)
        for name, n_remove, n_append in (("1_appended", 0, 1), ("1_removed", 1, 0), ("32_removed_32_appended", 32, 32),
                                         ("1pct_removed_and_appended", one_percent, one_percent)):
            call, call_b, load, load_b, dropped, missing = [], [], [], [], 0, 0
            for _ in range(reps):
                remove = np.sort(rng.choice(g, n_remove, replace=False)).astype(np.uint32)
                src = rng.integers(0, g, n_append)
                rows = soa.Groups(*[getattr(groups, n)[..., src] for n in COLUMNS])
                for through in (False, True):
                    fresh(ctx, nodes, fit, groups, pods, bound)
                    t = time.perf_counter()
                    r = ctx.groups_list_apply(remove, [], rows, n_append, wait_cap=0)
                    if through:
                        first_batch(ctx)
                    (call_b if through else call).append(time.perf_counter() - t)
                    dropped, missing = r["n_wait_dropped"], r["n_pods_missing"]
                    fresh(ctx, nodes, fit, groups, pods, bound)
                    new_groups, imap = new_list(ctx.read_groups(), remove, rows), index_map(g, remove)      # the caller's list: outside the timed region
                    spent = reload_path(ctx, new_groups, imap, pods, bound, sync)
                    if through:
                        t = time.perf_counter()
                        first_batch(ctx)
                        spent += time.perf_counter() - t
                    (load_b if through else load).append(spent)
            us = lambda v: {"best": min(v) * 1e6, "median": float(np.median(v)) * 1e6}
            out["modes"][name] = {"removed": n_remove, "appended": n_append, "wait_rows_dropped_last_rep": dropped, "pods_missing_last_rep": missing,
                                  "list_apply_us": us(call), "reload_path_us": us(load), "list_apply_to_first_map_us": us(call_b),
                                  "reload_path_to_first_map_us": us(load_b)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
