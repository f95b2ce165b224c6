"""Times bs_preempt_run (the batched gang-aware victim search, csrc/bs_preempt.hpp) at the cfg3 and cfg4 node counts with 20-110 bound
pods per node, for 64 and 1024 preemptors.  Prints one JSON line: ms per call (median of --reps calls after --warmup), end to end
through the C ABI (upload of the preemptor arrays, both launches, the result copy).  --commit times bs_preempt_commit instead (the
plan answered in sequence, distinct preemptors) with flags 0 and BS_PREEMPT_APPLY; an APPLY call is timed from the state as loaded (the
nodes and the bound table are reloaded, untimed, before every call).  --pdb FRACTION marks that share of the bound pods (seeded) as
PDB-violating through bs_bound_pdb_set before the timed calls; the default 0 sets no bits.  --bound-apply K [K ...] times the bound
table's patch instead: bs_bound_apply with K removes (seeded live ids) + K inserts (seeded nodes), next to bs_bound_load of a table of
the same size (what a caller without the patch pays per event batch) and to a plain device-to-device copy of the table's allocation (the
floor of any patch that forms a copy), all in one process.  --nodes times bs_bound_nodes_apply (the table follows node-list surgery) for one
remove + one append and for 16 removes, each next to bs_bound_load of the equivalent table (what the call replaces) in alternating order,
and next to bs_bound_apply with 64 removes + 64 inserts on the same table.  --bound-nodes K times bs_bound_apply_ex with BS_BOUND_NODES (K removes +
K inserts: table and node requests in one call) against the sequence it replaces, in alternating order on one context: the new absolute
request vectors of the touched nodes computed on the host (numpy, from a host copy of the entries' requests), bs_bound_apply, then
bs_nodes_assume; the three parts are also reported on their own.  --pdb-resident times one bs_pdb_allowed_apply of 8 indices (64 resident
PDBs, the bits recomputed on the device) and, in the same process, the path it replaces, its two parts reported separately:
pdb.violating_bits over string records of every bound pod, then bs_bound_pdb_set.  --gang FRACTION times bs_preempt_commit_gang (plan only)
on cfg3 at 64 and 1024 preemptors listed in gang_order, with every need 0 and with needs drawn so that FRACTION of the runs that place
a member miss their quorum by one (a run that places nobody misses its need of 1 anyway; the row reports the runs that missed in all), beside bs_preempt_commit on the same list in the same process: the plain call five times over (median of --reps calls
each; their spread is the yardstick's noise), the three calls taking turns.  --nominated-nodes times bs_nominated_nodes_apply (the
nominated-pod table follows node-list surgery) on the cfg3 node list with a table of 4096 rows, for 1 node removed, 32 removed, and 1 % of
the nodes removed with as many appended, beside the path it replaces on the same context: bs_nominated_read (before the surgery), a numpy
remap of the node column, bs_nominated_load; bs_nodes_apply itself is untimed (both paths need it) and every timed call starts from the
table as loaded.  --commit --clear times bs_preempt_commit with BS_PREEMPT_CLEAR_LOWER beside the same call without the flag, on one context
with a populated nominated-pod table (--nominated FRACTION, 0.5 when not given), the two calls taking turns, with flags 0 and with
BS_PREEMPT_APPLY (nodes, bound table and nominated-pod table reloaded, untimed, before every APPLY call); the row reports the cleared rows."""
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


def load_nominated(ctx, fraction: float, n: int, pods, prio, L: int) -> int:
    """--nominated: `fraction` of the nodes hold one row of the resident nominated-pod table each (bs_nominated_load); the rows' requests
    are those of queue pods, their priorities are drawn from the preemptors' (so a row counts for some preemptors and not for others).
    Returns the row count."""
    rng = np.random.default_rng(20260921 ^ 0x40B)
    node = np.nonzero(rng.random(n) < fraction)[0].astype(np.uint32)
    src = rng.integers(0, pods.p, size=node.size)
    ctx.nominated_load(node, np.asarray(prio)[rng.integers(0, len(prio), size=node.size)], pods.req[:L, src], pods.req_present[src])
    return int(node.size)


def one(config: str, q: int, reps: int, warmup: int, commit: bool = False, apply: bool = False, pdb: float = 0.0, nominated: float = 0.0) -> dict:
    cfg = synth.CONFIGS[config]
    n, S = cfg["nodes"], cfg["scalars"]
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    pods, pidx, prio = synth.make_preemptors(20260921, q, 4096, cfg["groups"], S, cfg["classes"])
    if commit:                                             # a pod is nominated once
        pidx = np.random.default_rng(20260921).permutation(4096)[:q].astype(np.uint32)
    groups = soa.Groups.empty(cfg["groups"], 4 + S)
    prot = (synth.Stream(20260921, 99).uniform(cfg["groups"]) < 0.3).astype(np.uint8)
    bits = (np.random.default_rng(20260921).random(bound.b) < pdb).astype(np.uint8) if pdb > 0 else None
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        ctx.load_bound(bound)
        if bits is not None:
            ctx.bound_pdb_set(bits)
        rows = load_nominated(ctx, nominated, n, pods, prio, 4 + S) if nominated > 0 else 0
        def call():
            if not commit:
                return ctx.preempt(pidx, prio, prot, victim_cap=16)
            return ctx.preempt_commit(pidx, prio, prot, victim_cap=16, apply=apply)

        ts = []
        for it in range(warmup + reps):
            if apply and it:
                ctx.load_nodes(nodes, fit)
                ctx.load_bound(bound)
                if bits is not None:
                    ctx.bound_pdb_set(bits)
            t0 = time.perf_counter()
            r = call()
            if it >= warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
    row = dict(config=config, nodes=n, bound=int(bound.b), preemptors=q, ms=round(float(np.median(ts)), 4), ms_min=round(float(min(ts)), 4),
               placed=int((r["node"] >= 0).sum()), with_victims=int((r["n_victims"] > 0).sum()))
    if pdb > 0:
        row.update(pdb=pdb, pdb_violations=int(r["n_pdb_violations"].sum()))
    if commit:
        row.update(flags="APPLY" if apply else "0", evicted=int(r["n_victims"].sum()))
    if nominated > 0:
        row.update(nominated=nominated, nominated_rows=rows)
    return row


def clear_rows(config: str, q: int, reps: int, warmup: int, apply: bool, nominated: float) -> dict:
    """--commit --clear: the flagged call and the flag-less call in turns on the scene of `one` (commit) with a populated table"""
    cfg = synth.CONFIGS[config]
    n, S = cfg["nodes"], cfg["scalars"]
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    pods, _, prio = synth.make_preemptors(20260921, q, 4096, cfg["groups"], S, cfg["classes"])
    pidx = np.random.default_rng(20260921).permutation(4096)[:q].astype(np.uint32)
    groups = soa.Groups.empty(cfg["groups"], 4 + S)
    prot = (synth.Stream(20260921, 99).uniform(cfg["groups"]) < 0.3).astype(np.uint8)
    ts = {False: [], True: []}
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        ctx.load_bound(bound)
        rows = load_nominated(ctx, nominated, n, pods, prio, 4 + S)
        res, ts_started = {}, False
        for it in range(warmup + reps):
            for flagged in ((False, True) if it % 2 == 0 else (True, False)):
                if apply and ts_started:                     # (the first call of all starts from the state as loaded above)
                    ctx.load_nodes(nodes, fit)
                    ctx.load_bound(bound)
                    load_nominated(ctx, nominated, n, pods, prio, 4 + S)
                ts_started = True
                t0 = time.perf_counter()
                res[flagged] = ctx.preempt_commit(pidx, prio, prot, victim_cap=16, apply=apply, clear_lower=flagged)
                if it >= warmup:
                    ts[flagged].append((time.perf_counter() - t0) * 1e3)
    med = lambda v: round(float(np.median(v)), 4)            # noqa: E731
    r0, r1 = res[False], res[True]
    return dict(config=config, nodes=n, bound=int(bound.b), preemptors=q, flags="APPLY" if apply else "0", nominated=nominated, nominated_rows=rows,
                ms=med(ts[False]), ms_min=round(float(min(ts[False])), 4), clear_ms=med(ts[True]), clear_ms_min=round(float(min(ts[True])), 4),
                clear_over_plain=round(med(ts[True]) / med(ts[False]), 3), cleared=int(r1["cleared"]["id"].size),
                placed=int((r0["node"] >= 0).sum()), clear_placed=int((r1["node"] >= 0).sum()), evicted=int(r0["n_victims"].sum()),
                clear_evicted=int(r1["n_victims"].sum()))


def _table_bytes(L: int, n: int, b: int) -> int:
    """the size of the bound table's one allocation (csrc/bs_kernels.hpp, bound_layout: columns at 256-byte offsets)"""
    al = lambda x: (x + 255) // 256 * 256                     # noqa: E731
    nb = max(b, 1)
    return sum(al(x) for x in ((n + 1) * 4, nb * 4, nb * 8, nb * 4, nb * 4, nb * L * 8, nb * 4, nb, max(n, 1) * 4))


def _median_ms(fn, reps: int, warmup: int) -> tuple:
    ts = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 4), round(float(min(ts)), 4)


def bound_apply_rows(config: str, ks, reps: int, warmup: int) -> list:
    import torch
    cfg = synth.CONFIGS[config]
    n, S = cfg["nodes"], cfg["scalars"]
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    rng = np.random.default_rng(20260921)
    rows = []
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_bound(bound)
        nbytes = _table_bytes(4 + S, n, bound.b)
        src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()

        copy_ms, copy_min = _median_ms(copy, reps, warmup)
        load_ms, load_min = _median_ms(lambda: ctx.load_bound(bound), reps, warmup)
        for k in ks:
            ctx.load_bound(bound)
            live = np.arange(bound.b, dtype=np.uint32)
            ts = []
            for it in range(warmup + reps):
                at = rng.permutation(live.size)[:k]
                src_i = rng.integers(0, bound.b, k)
                ins = soa.Bound(rng.integers(0, n, k).astype(np.uint32), bound.priority[src_i], bound.start_ns[src_i], bound.group[src_i],
                                bound.req[:, src_i], bound.req_present[src_i])
                rem = live[at]
                t0 = time.perf_counter()
                first = ctx.bound_apply(rem, ins)
                if it >= warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
                live = np.concatenate([np.delete(live, at), np.arange(first, first + k, dtype=np.uint32)])
            assert ctx.bound_count() == bound.b and np.array_equal(np.sort(ctx.read_bound()[0]), np.sort(live))
            ms = round(float(np.median(ts)), 4)
            rows.append(dict(config=config, nodes=n, bound=int(bound.b), table_bytes=nbytes, k=k, apply_ms=ms, apply_ms_min=round(float(min(ts)), 4),
                             reload_ms=load_ms, reload_ms_min=load_min, copy_ms=copy_ms, copy_ms_min=copy_min,
                             reload_over_apply=round(load_ms / ms, 2), apply_over_copy=round(ms / copy_ms, 2)))
    return rows


def bound_nodes_rows(config: str, reps: int, warmup: int) -> list:
    capi = bsa.capi
    cfg = synth.CONFIGS[config]
    n, S = cfg["nodes"], cfg["scalars"]
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    rng = np.random.default_rng(20260921)

    def delta(kind, index):
        d = capi.NodeDelta()
        d.kind, d.index, d.fit_default = kind, int(index), 1
        if kind == capi.DELTA_APPEND:                          # a copy of node 0, empty
            for j in range(4 + S):
                d.allocatable[j] = int(nodes.allocatable[j, 0])
            d.allocatable_present = int(nodes.allocatable_present[0])
        return d

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    rows = []
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_bound(bound)
        ts = []
        for it in range(warmup + reps):                        # bs_bound_apply, 64 + 64, on the same table
            src_i = rng.integers(0, bound.b, 64)
            ins = soa.Bound(rng.integers(0, n, 64).astype(np.uint32), bound.priority[src_i], bound.start_ns[src_i], bound.group[src_i],
                            bound.req[:, src_i], bound.req_present[src_i])
            rem = ctx.read_bound()[0][rng.permutation(bound.b)[:64]]
            ts.append(timed(lambda: ctx.bound_apply(rem, ins)))
        apply_ms = float(np.median(ts[warmup:]))
        for case, n_rem, n_app in (("1 remove + 1 append", 1, 1), ("16 removes", 16, 0)):
            ctx.load_nodes(nodes, fit)
            ctx.load_bound(bound)
            cur, cur_n = bound, n

            def surgery():
                """one list surgery on the node list (untimed); returns (kinds, indices, the equivalent table after it)"""
                nonlocal cur, cur_n
                labels = np.arange(cur_n)
                deltas = []
                for _ in range(n_rem):
                    i = int(rng.integers(0, labels.size))
                    labels = np.delete(labels, i)
                    deltas.append(delta(capi.DELTA_REMOVE, i))
                deltas += [delta(capi.DELTA_APPEND, 0) for _ in range(n_app)]
                ctx.apply_node_deltas(deltas)
                new_of_old = np.full(cur_n, -1, np.int64)
                new_of_old[labels] = np.arange(labels.size)
                keep = new_of_old[cur.node] >= 0
                cur = soa.Bound(new_of_old[cur.node[keep]].astype(np.uint32), cur.priority[keep], cur.start_ns[keep], cur.group[keep],
                                cur.req[:, keep], cur.req_present[keep])
                cur_n = labels.size + n_app
                return [d.kind for d in deltas], [d.index for d in deltas]

            t_nodes, t_load, dropped = [], [], 0
            for it in range(warmup + reps):
                kinds, idx = surgery()
                if it % 2:                                     # the reload first; the call then follows a second surgery
                    t_load.append(timed(lambda: ctx.load_bound(cur)))
                    kinds, idx = surgery()
                before = ctx.bound_count()
                t_nodes.append(timed(lambda: ctx.bound_nodes_apply(kinds, idx)))
                dropped += before - ctx.bound_count()
                if not it % 2:
                    t_load.append(timed(lambda: ctx.load_bound(cur)))
            assert ctx.bound_count() == cur.b and ctx.n == cur_n and np.array_equal(np.sort(ctx.read_bound()[1]), np.sort(cur.node))
            ms, load_ms = float(np.median(t_nodes[warmup:])), float(np.median(t_load[warmup:]))
            rows.append(dict(config=config, nodes=n, bound=int(bound.b), case=case, nodes_apply_ms=round(ms, 4), nodes_apply_ms_min=round(min(t_nodes[warmup:]), 4),
                             reload_ms=round(load_ms, 4), reload_ms_min=round(min(t_load[warmup:]), 4), bound_apply_64_64_ms=round(apply_ms, 4),
                             dropped_per_call=round(dropped / (warmup + reps), 1), reload_over_nodes_apply=round(load_ms / ms, 2),
                             nodes_apply_over_bound_apply=round(ms / apply_ms, 2)))
    return rows


def bound_apply_nodes_rows(config: str, k: int, reps: int, warmup: int) -> list:
    import ctypes as C
    capi = bsa.capi
    cfg = synth.CONFIGS[config]
    n, S = cfg["nodes"], cfg["scalars"]
    L = 4 + S
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    rng = np.random.default_rng(20260921)
    smask = np.uint32((1 << S) - 1)

    def stored(b):                                             # the columns as the table stores them
        req = np.array(b.req, np.int64, copy=True)
        pres = b.req_present & smask
        req[3] = 1
        for j in range(S):
            req[4 + j] = np.where((pres >> np.uint32(j)) & 1, req[4 + j], 0)
        return req, pres

    rec = np.dtype([("index", np.uint32), ("requested_present", np.uint32), ("requested", np.int64, (soa.MAX_LANES,))])
    assert rec.itemsize == C.sizeof(capi.NodeRequest)
    h_req, h_pres = stored(bound)                              # the shim's copy of every entry, by id
    h_node = bound.node.copy()
    n_req, n_pres = np.array(nodes.requested, np.int64, copy=True), np.array(nodes.requested_present, np.uint32, copy=True)
    t_ex, t_host, t_apply, t_assume = [], [], [], []
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_bound(bound)
        live = np.arange(bound.b, dtype=np.uint32)
        for it in range(2 * (warmup + reps)):
            at = rng.permutation(live.size)[:k]
            src_i = rng.integers(0, bound.b, k)
            ins = soa.Bound(rng.integers(0, n, k).astype(np.uint32), bound.priority[src_i], bound.start_ns[src_i], bound.group[src_i],
                            bound.req[:, src_i], bound.req_present[src_i])
            rem = live[at]
            t0 = time.perf_counter()                           # the host arithmetic of the two-call sequence (the flagged call needs none of it)
            ireq, ipres = stored(ins)
            d = np.zeros((L, n), np.int64)
            bits = np.zeros(n, np.uint32)
            with np.errstate(over="ignore"):
                for j in range(L):
                    np.subtract.at(d[j], h_node[rem], h_req[j, rem])
                    np.add.at(d[j], ins.node, ireq[j])
            np.bitwise_or.at(bits, h_node[rem], h_pres[rem])
            np.bitwise_or.at(bits, ins.node, ipres)
            hit = np.unique(np.concatenate([h_node[rem], ins.node]))
            for j in range(L):
                on = np.ones(hit.size, bool) if j < 4 else ((bits[hit] >> np.uint32(j - 4)) & 1) != 0
                base = n_req[j, hit] if j < 4 else np.where((n_pres[hit] >> np.uint32(j - 4)) & 1, n_req[j, hit], 0)
                with np.errstate(over="ignore"):
                    n_req[j, hit] = np.where(on, base + d[j, hit], n_req[j, hit])
            n_pres[hit] |= bits[hit]
            recs = np.zeros(hit.size, rec)
            recs["index"], recs["requested_present"] = hit, n_pres[hit]
            recs["requested"][:, :L] = n_req[:, hit].T
            t1 = time.perf_counter()
            timed = it >= 2 * warmup
            if it % 2:
                first = ctx.bound_apply(rem, ins)
                t2 = time.perf_counter()
                ctx._chk(ctx._lib.bs_nodes_assume(ctx._h, recs.ctypes.data_as(C.POINTER(capi.NodeRequest)), int(hit.size)), "bs_nodes_assume")
                t3 = time.perf_counter()
                if timed:
                    t_host.append((t1 - t0) * 1e3), t_apply.append((t2 - t1) * 1e3), t_assume.append((t3 - t2) * 1e3)
            else:
                first = ctx.bound_apply_ex(rem, ins, flags=capi.BS_BOUND_NODES)
                if timed:
                    t_ex.append((time.perf_counter() - t1) * 1e3)
            h_req, h_pres, h_node = np.concatenate([h_req, ireq], axis=1), np.concatenate([h_pres, ipres]), np.concatenate([h_node, ins.node])
            live = np.concatenate([np.delete(live, at), np.arange(first, first + k, dtype=np.uint32)])
        got_req, got_pres = ctx.read_node_requests()
        assert np.array_equal(got_req, n_req) and np.array_equal(got_pres, n_pres), "the two forms left different node requests"
    med = lambda t: round(float(np.median(t)), 4)              # noqa: E731
    two = [a + b + c for a, b, c in zip(t_host, t_apply, t_assume)]
    return [dict(config=config, nodes=n, bound=int(bound.b), k=k, flagged_ms=med(t_ex), flagged_ms_min=round(min(t_ex), 4), two_call_ms=med(two),
                 two_call_ms_min=round(min(two), 4), host_vectors_ms=med(t_host), bound_apply_ms=med(t_apply), nodes_assume_ms=med(t_assume),
                 two_calls_without_host_ms=med([b + c for b, c in zip(t_apply, t_assume)]), two_call_over_flagged=round(med(two) / med(t_ex), 2))]


def pdb_resident_rows(config: str, reps: int, warmup: int, host_reps: int = 2) -> list:
    pdbmod = bsa.pdb
    cfg = synth.CONFIGS[config]
    n, S, n_pdb = cfg["nodes"], cfg["scalars"], 64
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    rng = np.random.default_rng(20260921)
    app = rng.integers(0, n_pdb + 16, bound.b)                 # PDB m selects app=a<m>: a fifth of the pods are selected by nobody
    pods = [{"namespace": "default", "labels": {"app": f"a{j}"}} for j in app.tolist()]
    allowed = np.where(rng.random(n_pdb) < 0.1, 0, 2).astype(np.int32)
    pdbs = [{"namespace": "default", "selector": {"matchLabels": {"app": f"a{m}"}}, "disruptions_allowed": int(v)} for m, v in enumerate(allowed)]
    sel = app < n_pdb                                          # the memberships, as matching_members gives them (held against it on a sample)
    off = np.concatenate([[0], np.cumsum(sel)]).astype(np.uint32)
    member = app[sel].astype(np.uint32)
    s_off, s_member = pdbmod.matching_members(pdbs, pods[:2000])
    assert np.array_equal(s_off, off[:2001]) and np.array_equal(s_member, member[: int(off[2000])])
    t_apply, t_bits, t_set = [], [], []
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_bound(bound)
        ctx.pdb_load(allowed, off, member)
        ids, _ = ctx.read_bound()
        for it in range(warmup + reps):
            idx = rng.permutation(n_pdb)[:8]
            val = np.where(allowed[idx] <= 0, 2, 0).astype(np.int32)
            t0 = time.perf_counter()
            ctx.pdb_allowed_apply(idx, val)
            if it >= warmup:
                t_apply.append((time.perf_counter() - t0) * 1e3)
            allowed[idx] = val
        resident = ctx.bound_dump()["pdb"]
        for m, v in enumerate(allowed):
            pdbs[m]["disruptions_allowed"] = int(v)
        for it in range(host_reps):                            # the replaced path, on the same context (the last writer wins)
            t0 = time.perf_counter()
            bits = pdbmod.violating_bits(pdbs, pods)
            t1 = time.perf_counter()
            ctx.bound_pdb_set(bits)
            t_bits.append((t1 - t0) * 1e3), t_set.append((time.perf_counter() - t1) * 1e3)
        assert np.array_equal(resident, bits[ids]) and np.array_equal(ctx.bound_dump()["pdb"], resident), "the two paths left different bits"
    med = lambda t: round(float(np.median(t)), 4)              # noqa: E731
    return [dict(config=config, nodes=n, bound=int(bound.b), pdbs=n_pdb, members=int(member.size), indices=8, allowed_apply_ms=med(t_apply),
                 allowed_apply_ms_min=round(min(t_apply), 4), violating_bits_ms=med(t_bits), bound_pdb_set_ms=med(t_set),
                 bound_pdb_set_ms_min=round(min(t_set), 4), violating=int(resident.sum()),
                 pdb_set_over_allowed_apply=round(med(t_set) / med(t_apply), 2))]


def gang_rows(config: str, q: int, fraction: float, reps: int, warmup: int, nominated: float = 0.0) -> list:
    capi = bsa.capi
    cfg = synth.CONFIGS[config]
    n, S = cfg["nodes"], cfg["scalars"]
    bound, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    pods, _, prio = synth.make_preemptors(20260921, q, 4096, cfg["groups"], S, cfg["classes"])
    rng = np.random.default_rng(20260921)
    pidx = rng.permutation(4096)[:q].astype(np.uint32)
    grp = np.asarray(pods.group)[pidx].astype(np.int64)
    prio = prio.astype(np.int64)
    for g in np.unique(grp[grp >= 0]):                         # one priority a gang: gang_order then makes it one run
        prio[grp == g] = prio[grp == g][0]
    o = capi.gang_order(grp, prio)
    pidx, prio, grp = pidx[o], prio[o].astype(np.int32), grp[o]
    groups = soa.Groups.empty(cfg["groups"], 4 + S)
    prot = (synth.Stream(20260921, 99).uniform(cfg["groups"]) < 0.3).astype(np.uint8)
    zero = np.zeros(cfg["groups"], np.uint32)
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        ctx.load_bound(bound)
        nom_rows = load_nominated(ctx, nominated, n, pods, prio, 4 + S) if nominated > 0 else 0
        # what each gang places when every run stands; a share of the gangs that place something then ask for one more than that
        one_each = np.zeros(cfg["groups"], np.uint32)
        one_each[np.unique(grp[grp >= 0])] = 1
        placed = ctx.preempt_commit_gang(pidx, prio, prot, one_each, victim_cap=16)["group_placed"]
        can = np.nonzero(placed > 0)[0]
        miss = can[rng.random(can.size) < fraction]
        need = np.where(one_each > 0, np.maximum(placed, 1), 0).astype(np.uint32)
        need[miss] = placed[miss] + 1
        calls = dict(plain=lambda: ctx.preempt_commit(pidx, prio, prot, victim_cap=16),
                     gang0=lambda: ctx.preempt_commit_gang(pidx, prio, prot, zero, victim_cap=16),
                     gang=lambda: ctx.preempt_commit_gang(pidx, prio, prot, need, victim_cap=16))
        ts = {k: [] for k in calls}
        for it in range(warmup + 5 * reps):                    # the three take turns; the plain call's samples are cut into five repeats
            for k, fn in calls.items():
                if k != "plain" and it >= warmup + reps:
                    continue
                t0 = time.perf_counter()
                r = fn()
                if it >= warmup:
                    ts[k].append((time.perf_counter() - t0) * 1e3)
                if k == "gang":
                    last = r
        r = last
        runs = int((need > 0).sum())
        missed = int(((need > 0) & (r["group_placed"] < need)).sum())
        voided = int(r["slot_voided"].sum())
    five = [float(np.median(ts["plain"][i * reps:(i + 1) * reps])) for i in range(5)]
    plain, g0, g1 = float(np.median(five)), float(np.median(ts["gang0"])), float(np.median(ts["gang"]))
    return [dict(config=config, nodes=n, bound=int(bound.b), preemptors=q, runs=runs, missed_runs=missed, voided_slots=voided, fraction=fraction,
                 plain_ms=round(plain, 4), plain_five=[round(x, 4) for x in five], plain_spread_ms=round(max(five) - min(five), 4),
                 gang_need0_ms=round(g0, 4), gang_ms=round(g1, 4), need0_over_plain=round(g0 / plain, 4), gang_over_plain=round(g1 / plain, 4),
                 **(dict(nominated=nominated, nominated_rows=nom_rows) if nominated > 0 else {}))]


def nominated_nodes_rows(reps: int, warmup: int, table_rows: int = 4096) -> list:
    capi = bsa.capi
    cfg = synth.CONFIGS["cfg3"]
    n, S = cfg["nodes"], cfg["scalars"]
    _, nodes = synth.make_bound(20260921, n, cfg["groups"], (20, 110), S)
    fit = synth.make_fit(20260921, n, cfg["classes"])
    pods, _, prio = synth.make_preemptors(20260921, 64, 4096, cfg["groups"], S, cfg["classes"])
    rng = np.random.default_rng(20260921 ^ 0x40B)
    src = rng.integers(0, pods.p, size=table_rows)
    t_node = rng.integers(0, n, size=table_rows).astype(np.uint32)
    t_prio, t_req, t_pres = np.asarray(prio)[rng.integers(0, len(prio), size=table_rows)], pods.req[: 4 + S, src], pods.req_present[src]

    def delta(kind, index):
        d = capi.NodeDelta()
        d.kind, d.index, d.fit_default = kind, int(index), 1
        if kind == capi.DELTA_APPEND:                          # a copy of node 0, empty
            for j in range(4 + S):
                d.allocatable[j] = int(nodes.allocatable[j, 0])
            d.allocatable_present = int(nodes.allocatable_present[0])
        return d

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    rows = []
    with bsa.Context(scalar_lanes=S, device=0) as ctx:
        for case, n_rem, n_app in (("1 node removed", 1, 0), ("32 nodes removed", 32, 0), ("1 % removed, as many appended", n // 100, n // 100)):
            def reload():
                ctx.load_nodes(nodes, fit)
                ctx.nominated_load(t_node, t_prio, t_req, t_pres)

            def surgery():
                """one list surgery from the node list as loaded (untimed) -> (kinds, indices, new index of every old node or -1)"""
                labels = np.arange(n)
                deltas = []
                for _ in range(n_rem):
                    i = int(rng.integers(0, labels.size))
                    labels = np.delete(labels, i)
                    deltas.append(delta(capi.DELTA_REMOVE, i))
                deltas += [delta(capi.DELTA_APPEND, 0) for _ in range(n_app)]
                ctx.apply_node_deltas(deltas)
                new_of_old = np.full(n, -1, np.int64)
                new_of_old[labels] = np.arange(labels.size)
                return [d.kind for d in deltas], [d.index for d in deltas], new_of_old

            t_call, t_read, t_remap, t_load, dropped = [], [], [], [], 0
            for it in range(warmup + reps):
                reload()                                       # the path the call replaces: read, [surgery], remap on the host, load
                ms_read, cols = timed(ctx.nominated_read)
                kinds, idx, new_of_old = surgery()

                def remap():
                    new = new_of_old[cols["node"]]
                    keep = new >= 0
                    return new[keep].astype(np.uint32), cols["priority"][keep], np.ascontiguousarray(cols["req"][:, keep]), cols["req_present"][keep]
                ms_remap, host = timed(remap)
                ms_load, _ = timed(lambda: ctx.nominated_load(*host))
                reload()                                       # the call
                kinds, idx, new_of_old = surgery()
                ms_call, out = timed(lambda: ctx.nominated_nodes_apply(kinds, idx))
                assert out[3] == int((new_of_old[t_node] < 0).sum()) and ctx.nominated_count() == table_rows - out[3]
                dropped += out[3]
                if it >= warmup:
                    t_call.append(ms_call), t_read.append(ms_read), t_remap.append(ms_remap), t_load.append(ms_load)
            med = lambda v: float(np.median(v))                    # noqa: E731
            host_ms = med(np.array(t_read) + np.array(t_remap) + np.array(t_load))
            rows.append(dict(config="cfg3", nodes=n, table_rows=table_rows, case=case, removed=n_rem, appended=n_app,
                             nodes_apply_ms=round(med(t_call), 4), nodes_apply_ms_min=round(min(t_call), 4), read_remap_load_ms=round(host_ms, 4),
                             read_ms=round(med(t_read), 4), remap_ms=round(med(t_remap), 4), load_ms=round(med(t_load), 4),
                             dropped_per_call=round(dropped / (warmup + reps), 1), read_remap_load_over_nodes_apply=round(host_ms / med(t_call), 2)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", action="store_true", help="bs_preempt_commit, flags 0 and APPLY")
    ap.add_argument("--pdb", type=float, default=0.0, metavar="FRACTION", help="share of the bound pods with the PDB-violating bit (seeded)")
    ap.add_argument("--bound-apply", type=int, nargs="+", default=None, metavar="K", help="bs_bound_apply with K removes + K inserts, vs the reload and a plain copy")
    ap.add_argument("--nodes", action="store_true", help="bs_bound_nodes_apply after 1 remove + 1 append and after 16 removes, vs the reload and bs_bound_apply")
    ap.add_argument("--bound-nodes", type=int, default=None, metavar="K", help="bs_bound_apply_ex(BS_BOUND_NODES) with K removes + K inserts, vs bs_bound_apply + "
                    "bs_nodes_assume with the vectors computed on the host")
    ap.add_argument("--pdb-resident", action="store_true", help="bs_pdb_allowed_apply of 8 indices, vs pdb.violating_bits + bs_bound_pdb_set")
    ap.add_argument("--gang", type=float, default=None, metavar="FRACTION", help="bs_preempt_commit_gang on cfg3 (need 0, and FRACTION of the runs missing "
                    "their quorum) beside bs_preempt_commit")
    ap.add_argument("--nominated", type=float, default=0.0, metavar="FRACTION", help="share of the nodes that hold one row of the nominated-pod table "
                    "(priorities drawn from the preemptors'); with the default scene, --commit and --gang")
    ap.add_argument("--clear", action="store_true", help="with --commit: BS_PREEMPT_CLEAR_LOWER beside the flag-less call on a populated nominated-pod table")
    ap.add_argument("--nominated-nodes", action="store_true", help="bs_nominated_nodes_apply on cfg3 with 4096 rows (1 node removed, 32 removed, 1 %% "
                    "removed with as many appended), vs bs_nominated_read + a numpy remap + bs_nominated_load")
    a = ap.parse_args()
    if a.nominated_nodes:
        print(json.dumps(dict(metric="bs_nominated_nodes_apply ms per call", rows=nominated_nodes_rows(a.reps, a.warmup))))
        return
    if a.gang is not None:
        rows = [r for q in (64, 1024) for r in gang_rows("cfg3", q, a.gang, a.reps, a.warmup, a.nominated)]
        print(json.dumps(dict(metric="bs_preempt_commit_gang ms per call", rows=rows)))
        return
    if a.pdb_resident:
        rows = [r for c in ("cfg3", "cfg4") for r in pdb_resident_rows(c, a.reps, a.warmup)]
        print(json.dumps(dict(metric="bs_pdb_allowed_apply ms per call", rows=rows)))
        return
    if a.bound_nodes:
        rows = [r for c in ("cfg3", "cfg4") for r in bound_apply_nodes_rows(c, a.bound_nodes, a.reps, a.warmup)]
        print(json.dumps(dict(metric="bs_bound_apply_ex ms per call", rows=rows)))
        return
    if a.nodes:
        rows = [r for c in ("cfg3", "cfg4") for r in bound_nodes_rows(c, a.reps, a.warmup)]
        print(json.dumps(dict(metric="bs_bound_nodes_apply ms per call", rows=rows)))
        return
    if a.bound_apply:
        rows = [r for c in ("cfg3", "cfg4") for r in bound_apply_rows(c, a.bound_apply, a.reps, a.warmup)]
        print(json.dumps(dict(metric="bs_bound_apply ms per call", rows=rows)))
        return
    if a.commit and a.clear:
        rows = [clear_rows(c, q, a.reps, a.warmup, ap_, a.nominated or 0.5) for c in ("cfg3", "cfg4") for q in (64, 1024) for ap_ in (False, True)]
        print(json.dumps(dict(metric="bs_preempt_commit with BS_PREEMPT_CLEAR_LOWER ms per call", rows=rows)))
        return
    if a.commit:
        rows = [one(c, q, a.reps, a.warmup, True, ap_, a.pdb, a.nominated) for c in ("cfg3", "cfg4") for q in (64, 1024) for ap_ in (False, True)]
        print(json.dumps(dict(metric="bs_preempt_commit ms per call", rows=rows)))
        return
    rows = [one(c, q, a.reps, a.warmup, pdb=a.pdb, nominated=a.nominated) for c in ("cfg3", "cfg4") for q in (64, 1024)]
    print(json.dumps(dict(metric="bs_preempt_run ms per call", rows=rows)))


if __name__ == "__main__":
    main()
