"""bs_wait_expire timed on a table the size of a cfg3 pass's waiting pods: 1 gang, 32 gangs and every gang of the table, beside the path it
replaces — the caller keeps its own copies of the waiting pods' requests and of the node requests, subtracts on the host (vectorised
numpy), hands the touched nodes to bs_nodes_assume and the groups to bs_groups_apply, then waits for the stream.  bs_wait_park is timed
too, after the same pass.  One untimed park + expire first, so that no figure contains the new kernels' code-object load.  Every figure is
the wall time of the call(s) as the caller sees them, best and median of `--reps` runs, each on a freshly loaded context that ran the pass
and parked.  No threshold is set.  Usage: python tools/wait_bench.py [config] [scenario] [--reps N] [--nodes]

--nodes times bs_wait_nodes_apply instead, on the same table, after a bs_nodes_apply (untimed: both paths need it) of three churn shapes —
1 node removed, 32 nodes removed, 1 % of the nodes removed plus as many appended; the nodes are drawn by a seeded generator of this tool —
beside the path the call replaces: bs_wait_read before the surgery, the remap in vectorised numpy (the removed nodes sorted, a searchsorted
per row), bs_wait_load of the survivors and the bs_groups_apply that takes the dropped rows off `matched`, then the stream.  The replaced
path's list of removed nodes and its copy of the groups are prepared outside its timed region; the call's replay of the delta list is
inside its own."""
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
soa, capi = bsa.soa, bsa.capi


def fresh(ctx, nodes, fit, groups, pods, park=True):
    """-> seconds bs_wait_park took (None when not asked to park)"""
    ctx.load_nodes(nodes, fit)
    ctx.load_groups(groups)
    ctx.load_pods(pods)
    ctx.seq_run(soa.STAGE_PREFILTER)
    ctx.wait_load()
    if not park:
        return None
    t = time.perf_counter()
    ctx.wait_park(cap=0)
    return time.perf_counter() - t


def host_path(ctx, tab, req, pres, grp, gangs, deny, sync):
    """what a shim does without the table on the device: subtract the gangs' rows from its own copy of the node requests (np.subtract.at),
    bs_nodes_assume of the touched nodes, bs_groups_apply of the gangs (matched 0, the deny bit), wait for the stream"""
    S = req.shape[0] - 4
    t = time.perf_counter()
    mine = np.nonzero(np.isin(tab["group"], gangs))[0]
    on = tab["node"][mine]
    touched = np.unique(on)
    req = req.copy()
    for j in range(4):
        np.subtract.at(req[j], on, tab["req"][j, mine])
    for s in range(S):
        has = ((tab["req_present"][mine] >> s) & 1) != 0
        np.subtract.at(req[4 + s], on[has], tab["req"][4 + s, mine[has]])
    cols = req[:, touched].T.tolist()
    ctx.assume_nodes(zip(touched.tolist(), cols, pres[touched].tolist()))
    ctx.apply_group_deltas([(int(g), 0, int(grp.status_scheduled[g]), int(grp.flags[g]) | (soa.GROUP_DENIED if deny else 0)) for g in gangs])
    sync()
    return time.perf_counter() - t


def node_delta(nodes, kind, index, like=0):
    """a REMOVE of `index`, or an APPEND of an empty node with the allocatable columns of node `like` that fits every class"""
    d = capi.NodeDelta()
    d.kind, d.index = int(kind), int(index)
    if kind == capi.DELTA_APPEND:
        for j in range(nodes.lanes):
            d.allocatable[j], d.requested[j] = int(nodes.allocatable[j, like]), 0
        d.allocatable_present, d.requested_present, d.flags, d.fit_default, d.n_fit_exceptions = int(nodes.allocatable_present[like]), 0, 0, 1, 0
    return d


def churn(nodes, rng, n_remove, n_append):
    """-> (deltas, the removed OLD nodes ascending): n_remove random nodes leave in a random order, then n_append nodes are appended"""
    old = rng.choice(nodes.n, n_remove, replace=False)
    gone, deltas = [], []
    for k in old.tolist():
        deltas.append(node_delta(nodes, capi.DELTA_REMOVE, k - sum(x < k for x in gone)))
        gone.append(k)
    deltas += [node_delta(nodes, capi.DELTA_APPEND, 0, int(rng.integers(0, nodes.n))) for _ in range(n_append)]
    return deltas, np.sort(old).astype(np.int64)


def replaced_path(ctx, deltas, rem, grp, sync):
    """bs_wait_read (before the surgery: afterwards the count is stale), [bs_nodes_apply, untimed], the remap on the host, bs_wait_load,
    bs_groups_apply for matched; -> (seconds, rows dropped)"""
    t = time.perf_counter()
    tab = ctx.wait_read()
    spent = time.perf_counter() - t
    ctx.apply_node_deltas(deltas)
    t = time.perf_counter()
    node = tab["node"].astype(np.int64)
    lo = np.searchsorted(rem, node)
    gone = np.isin(node, rem)
    keep = ~gone
    ctx.wait_load((node - lo)[keep], tab["group"][keep], tab["req"][:, keep], tab["req_present"][keep])
    fell = np.bincount(tab["group"][gone], minlength=grp.g)
    ctx.apply_group_deltas([(int(g), (int(grp.matched[g]) - int(fell[g])) & 0xFFFFFFFF, int(grp.status_scheduled[g]), int(grp.flags[g])) for g in np.nonzero(fell)[0]])
    sync()
    return spent + time.perf_counter() - t, int(gone.sum())


def nodes_mode(ctx, nodes, fit, groups, pods, reps, sync, out):
    rng = np.random.default_rng(5)
    one_percent = max(nodes.n // 100, 1)
    fresh(ctx, nodes, fit, groups, pods)
    d, _ = churn(nodes, rng, 1, 0)
    ctx.apply_node_deltas(d)
    ctx.wait_nodes_apply([x.kind for x in d], [x.index for x in d])           # warm-up: the first launch of the k_wn_* kernels loads their code
    for name, n_remove, n_append in (("1_removed", 1, 0), ("32_removed", 32, 0), ("1pct_removed_and_appended", one_percent, one_percent)):
        call, host, rows = [], [], 0
        for _ in range(reps):
            deltas, rem = churn(nodes, rng, n_remove, n_append)
            kinds, idx = [x.kind for x in deltas], [x.index for x in deltas]
            fresh(ctx, nodes, fit, groups, pods)
            ctx.apply_node_deltas(deltas)
            t = time.perf_counter()
            r = ctx.wait_nodes_apply(kinds, idx)
            call.append(time.perf_counter() - t)
            fresh(ctx, nodes, fit, groups, pods)
            spent, dropped = replaced_path(ctx, deltas, rem, ctx.read_groups(), sync)
            host.append(spent)
            assert dropped == r[3], (dropped, r[3])
            rows = r[3]
        out["modes"][name] = {"removed": n_remove, "appended": n_append, "rows_dropped_last_rep": rows,
                              "wait_nodes_apply_us_best": min(call) * 1e6, "wait_nodes_apply_us_median": float(np.median(call)) * 1e6,
                              "read_remap_load_us_best": min(host) * 1e6, "read_remap_load_us_median": float(np.median(host)) * 1e6}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    config = args[0] if args else "cfg3"
    scenario = args[1] if len(args) > 1 else "tail"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    nodes, fit, groups, pods, _ = bsa.synth.make(config, scenario)
    pods = pods.take(np.argsort(pods.group, kind="stable"))           # Compare order
    hip = C.CDLL("libamdhip64.so")
    out = {"config": f"{config}/{scenario}", "pods": int(pods.p), "nodes": int(nodes.n), "groups": int(groups.g), "reps": reps, "modes": {}}
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:
        stream = C.c_void_p(ctx.stream())
        sync = lambda: hip.hipStreamSynchronize(stream)
        if "--nodes" in sys.argv:
            fresh(ctx, nodes, fit, groups, pods)
            tab = ctx.wait_read()
            out["table_rows"], out["table_gangs"] = int(tab["id"].size), int(np.unique(tab["group"]).size)
            nodes_mode(ctx, nodes, fit, groups, pods, reps, sync, out)
            print(json.dumps(out))
            return
        fresh(ctx, nodes, fit, groups, pods)
        ctx.wait_expire(np.unique(ctx.wait_read()["group"]), deny=True, cap=0)      # warm-up: the first launch of the k_wt_* kernels loads their code object
        park = [fresh(ctx, nodes, fit, groups, pods) for _ in range(reps)]
        tab = ctx.wait_read()
        waiting = np.unique(tab["group"]).astype(np.uint32)
        out["table_rows"], out["table_gangs"] = int(tab["id"].size), int(waiting.size)
        out["park_us_best"], out["park_us_median"] = min(park) * 1e6, float(np.median(park)) * 1e6
        for name, gangs in (("1_gang", waiting[:1]), ("32_gangs", waiting[:: max(waiting.size // 32, 1)][:32]), ("all", waiting)):
            call, host, rows, n_nodes = [], [], 0, 0
            for _ in range(reps):
                fresh(ctx, nodes, fit, groups, pods)
                t = time.perf_counter()
                r = ctx.wait_expire(gangs, deny=True)
                call.append(time.perf_counter() - t)
                rows, n_nodes = r["n"], int(np.unique(r["node"]).size)
                fresh(ctx, nodes, fit, groups, pods)
                req, pres = ctx.read_node_requests()                    # the caller's own copies: outside the timed region
                host.append(host_path(ctx, tab, req, pres, ctx.read_groups(), gangs, True, sync))
            out["modes"][name] = {"gangs": int(len(gangs)), "rows": rows, "touched_nodes": n_nodes,
                                  "wait_expire_us_best": min(call) * 1e6, "wait_expire_us_median": float(np.median(call)) * 1e6,
                                  "host_path_us_best": min(host) * 1e6, "host_path_us_median": float(np.median(host)) * 1e6}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
