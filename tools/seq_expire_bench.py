"""bs_seq_expire timed after a sequential pass on a synthetic configuration: 1 gang, 32 gangs and every waiting gang (ALL), beside the
path the call replaces — bs_nodes_read + the subtraction on the host (vectorised numpy) + bs_nodes_apply(UPDATE) of the touched nodes,
then a stream wait — on the same state.  One untimed expire first, so that no figure contains the new kernels' code-object load.  Every
figure is the wall time of the call(s) as the caller sees them (the calls are synchronous), best and median of `--reps` runs, each on a freshly loaded context that ran the pass.  Usage: python tools/seq_expire_bench.py [config] [scenario] [--reps N]"""
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


def fresh(ctx, nodes, fit, groups, pods):
    ctx.load_nodes(nodes, fit)
    ctx.load_groups(groups)
    ctx.load_pods(pods)
    ctx.seq_run(soa.STAGE_PREFILTER)
    return ctx.seq_waiting_read()


def host_prepare(nodes, fitb):
    """per node, once and outside the timed region: a bs_node_delta with everything but the requests filled in (None where the node's
    fit row needs more than the 8 exceptions a delta holds)"""
    out = []
    for k in range(nodes.n):
        d = capi.NodeDelta()
        d.kind, d.index = capi.DELTA_UPDATE, k
        for j in range(nodes.lanes):
            d.allocatable[j] = int(nodes.allocatable[j, k])
        d.allocatable_present, d.flags = int(nodes.allocatable_present[k]), int(nodes.flags[k])
        on = np.nonzero(fitb[:, k])[0]
        d.fit_default, ex = (1, np.nonzero(~fitb[:, k])[0]) if on.size * 2 > fitb.shape[0] else (0, on)
        if ex.size > 8:
            out.append(None)
            continue
        d.n_fit_exceptions = int(ex.size)
        for e, c in enumerate(ex):
            d.fit_exceptions[e] = int(c)
        out.append(d)
    return out


def host_path(ctx, nodes, pods, wait, gangs, prepared, sync):
    """what a shim does without the call: read the node requests back, subtract the gangs' waiting pods (vectorised: np.subtract.at),
    write the touched nodes' request lanes into prepared deltas, bs_nodes_apply, wait for the stream.  What is left of Python in the timed
    region is the copy of L + 1 numbers into each touched node's delta and the binding's array of deltas."""
    S, L = nodes.lanes - 4, nodes.lanes
    mine = np.nonzero((wait >= 0) & np.isin(pods.group, gangs))[0]
    on = wait[mine]
    touched = np.unique(on)
    if any(prepared[k] is None for k in touched):
        return None
    t = time.perf_counter()
    req, pres = ctx.read_node_requests()
    req = req.copy()
    for j in range(3):
        np.subtract.at(req[j], on, pods.req[j, mine])
    np.subtract.at(req[3], on, 1)
    for s in range(S):
        has = ((pods.req_present[mine] >> s) & 1) != 0
        np.subtract.at(req[4 + s], on[has], pods.req[4 + s, mine[has]])
    cols = req[:, touched].T.tolist()
    bits = pres[touched].tolist()
    deltas = []
    for k, lanes, b in zip(touched.tolist(), cols, bits):
        d = prepared[k]
        d.requested[:L] = lanes
        d.requested_present = b
        deltas.append(d)
    if deltas:
        ctx.apply_node_deltas(deltas)
    sync()                                                         # (the apply is asynchronous: wait for it as the expire call waits)
    return time.perf_counter() - t


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    config = args[0] if args else "cfg3"
    scenario = args[1] if len(args) > 1 else "tail"
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7
    nodes, fit, groups, pods, _ = bsa.synth.make(config, scenario)
    pods = pods.take(np.argsort(pods.group, kind="stable"))           # Compare order
    prepared = host_prepare(nodes, fit.to_bool())
    hip = C.CDLL("libamdhip64.so")
    out = {"config": f"{config}/{scenario}", "pods": int(pods.p), "nodes": int(nodes.n), "groups": int(groups.g), "reps": reps, "modes": {}}
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:
        stream = C.c_void_p(ctx.stream())
        sync = lambda: hip.hipStreamSynchronize(stream)
        wait = fresh(ctx, nodes, fit, groups, pods)
        ctx.seq_expire(all=True)                                       # warm-up: the first launch of the k_se_* kernels loads their code object
        wait = fresh(ctx, nodes, fit, groups, pods)
        waiting = np.unique(pods.group[wait >= 0])
        out["waiting_gangs"], out["waiting_pods"] = int(waiting.size), int((wait >= 0).sum())
        for name, gangs in (("1_gang", waiting[:1]), ("32_gangs", waiting[:: max(waiting.size // 32, 1)][:32]), ("all", None)):
            call, host, n_pods, n_nodes = [], [], 0, 0
            for _ in range(reps):
                wait = fresh(ctx, nodes, fit, groups, pods)
                t = time.perf_counter()
                r = ctx.seq_expire(groups=gangs, deny=True, all=gangs is None)
                call.append(time.perf_counter() - t)
                n_pods, n_nodes = r["n_pods"], int(np.unique(r["node"]).size)
                wait = fresh(ctx, nodes, fit, groups, pods)
                h = host_path(ctx, nodes, pods, wait, waiting if gangs is None else gangs, prepared, sync)
                if h is not None:
                    host.append(h)
            out["modes"][name] = {"gangs": int(waiting.size if gangs is None else len(gangs)), "pods": n_pods, "touched_nodes": n_nodes,
                                  "expire_us_best": min(call) * 1e6, "expire_us_median": float(np.median(call)) * 1e6,
                                  "host_path_us_best": min(host) * 1e6 if host else None, "host_path_us_median": float(np.median(host)) * 1e6 if host else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
