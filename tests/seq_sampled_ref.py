"""Object-level model of the two sampled passes (TEST INFRASTRUCTURE): rule F of include/bsched.h over rule P (bs_seq_run_scored_sampled;
tests/seq_scored_ref.replay is the parent model) and over rule SP (bs_seq_run_scored_nominated_sampled; tests/seq_scored_nominated_ref.replay).
The replay loop is written out again.  For every pod that reaches the node choice the candidate set C of the form underneath is collected
in list order, exactly as the parent models collect it; the members are then ordered by VISIT POSITION from the cursor s — (k - s) mod N —,
the first K are kept (C'), the (K+1)-th, where there is one, ends the walk: V is its visit position, the nodes in front of it; otherwise
V = N.  The pod takes the member of C' with the largest seq_scored_ref.total_of over the node's own lanes, ties to the smallest visit
position, and the cursor moves by V.  D9 (numFeasibleNodesToFind) is stated here on Python ints.  Everything around the choice is the parent
models'."""
import naive_ref as nv
import naive_seq as ns
import seq_obj_replay as sor
from seq_nominated_ref import NOM_NONE, end_state_soa, objects_to_rows, with_rows  # noqa: F401  (the same objects and conversions)
from seq_scored_ref import WEIGHT_MAX, node_lanes, score_node, total_of  # noqa: F401

HAZARDS = "abcdefghijkl"        # the issue's list
EXTRA = "xm"                    # x: the K-th member sits in an EARLIER round than the (K+1)-th (the stopping wave has no kept member in front of the stop)
                                # m: with BS_STAGE_FILTER, the plugin's Filter removes the node that would have been the K-th member
WAVES = 8                       # tiles of 64 nodes per round of the kernel's walk (csrc/bs_seq.hpp, kSeqWaves)


def sample_size(n: int, percentage: int) -> int:
    """D9: upstream's numFeasibleNodesToFind; Python's // on non-negative ints truncates"""
    if n < 100 or percentage >= 100:
        return n
    a = percentage
    if a <= 0:
        a = max(50 - n // 125, 5)
    return max(n * a // 100, 100)


def norm_k(num_to_find: int, N: int) -> int:
    return N if num_to_find == 0 or num_to_find >= N else num_to_find


def position(s: int, k: int, N: int) -> int:
    return (k - s) % N


def slot(s: int, k: int, N: int) -> int:
    """the 64-lane slot of the kernel's walk that visits node k: slot u is tile (t_s + u) mod ntiles, t_s the cursor's tile; the nodes of that
    tile in front of the cursor are visited last, in a slot of their own behind the last tile"""
    ntiles = (N + 63) >> 6
    return (k >> 6) - (s >> 6) if k >= s else (k >> 6) + ntiles - (s >> 6)


def sample(C, s, K, N):
    """-> (kept [(visit position, node)] in visit order, V, the (K+1)-th member's (visit position, node) or None)"""
    order = sorted((position(s, k, N), k) for k in C)
    if len(order) > K:
        return order[:K], order[K][0], order[K]
    return order, N, None


def replay(sc, weights, sample_arg, closed=(), run_filter=False, scalar_names=(), nominees=None, priority=None, own_id=None):
    """sample_arg = (num_to_find, start).  nominees None: rule F over rule P (run_filter: BS_STAGE_FILTER narrows C); else rule F over
    rule SP with the nominated pods as objects, priority [p] and own_id [p] or None.
    -> seq_obj_replay.replay's dict plus total [p], n_fit [p] (= |C'|), assumed [p], start [p], visited [p], next_start, nominees and
    consumed (rule SP) and hazards, a count per letter:
    a: the choice differs from the full search's (the largest total over all of C, the lowest index); b: the maximum of C' is shared and the
    smallest visit position is not the lowest node index; c: the (K+1)-th member lies in the same slot of 64 lanes as the K-th; d: the
    (K+1)-th member lies behind the first round of 8 slots; e: it lies behind the wrap (its node index is below the cursor); f: it lies in
    the revisited low lanes of the cursor's tile; g: nodes that failed lie between the K-th and the (K+1)-th member; h: |C| == K exactly
    (K < N), so V = N; i: |C| < K (K < N); j: a pod that does not reach the choice finds a cursor that is not 0 and leaves it alone;
    k: under SP, a row removes a node from C and so moves the stop (V differs from the row-less walk's); l: under SP, an own row is
    consumed on a node that the full search would not have chosen."""
    assert all(0 <= w <= WEIGHT_MAX for w in weights) and len(weights) == 3
    sp = nominees is not None
    assert not (sp and run_filter), "the nominated form refuses BS_STAGE_FILTER"
    op = sor.build_operation(sc, closed)
    gnames = list(op.cache.keys())
    uid_index = {pod.uid: i for i, pod in enumerate(sc["pods"])}
    P, N = len(sc["pods"]), len(op.nodes)
    K = norm_k(int(sample_arg[0]), N)
    s = int(sample_arg[1]) % N if N else 0
    live, dead = list(nominees or []), []
    out = dict(pf_code=[], pf_first_k=[], pf_leader=[], pod_node=[-1] * P, released_group=[], released_pods=[], last_permitted=[0] * P)
    total, n_fit, assumed, consumed = [0] * P, [0] * P, [-1] * P, []
    start, visited = [0] * P, [0] * P
    hz = {c: 0 for c in HAZARDS + EXTRA}
    slot_of = {}
    for i, pod in enumerate(sc["pods"]):
        code, fk = op.prefilter(pod)
        out["pf_code"].append(code)
        out["pf_first_k"].append(fk)
        out["pf_leader"].append(gnames.index(op.max_finished_pg) if op.max_pg_status is not None else -1)
        own = NOM_NONE if own_id is None else int(own_id[i])
        if code >= 16 or (pod.group is not None and pod.group not in op.cache):
            hz["j"] += int(s != 0)
            if code < 16:
                assert op.permit(pod, pod.uid, 0) == (False, 3)
            continue
        req = nv.pod_resource_require(pod, True)
        req.ScalarResources = {k: v for k, v in (req.ScalarResources or {}).items() if k in scalar_names} or None
        # ---- C of the form underneath, in list order; raw: the same test without rows and without the plugin's Filter
        passes = None
        if run_filter:
            passes = []
            for k in range(N):
                inner = nv.ScheduleOperation(op.nodes, op.cache)
                inner.max_finished_pg, inner.max_pg_status = op.max_finished_pg, op.max_pg_status
                fl, fn = inner.filter_node(pod, k)
                passes.append(fl < 16 and (fl != nv.soa.FL_EVALUATED or fn < 16))
        C, raw = [], []
        for k, info in enumerate(op.nodes):
            if info.nil or not info.has_node or info.unschedulable or info.taint_err or not nv.check_fit(pod, info):
                continue
            ok_raw = sor.holds(info, req)
            if ok_raw:
                raw.append(k)
            if sp:
                mine = [o for o in live if o.node == k and o.id != own and o.priority >= int(priority[i])]
                ok = sor.holds(with_rows(info, mine), req) if mine else ok_raw
            else:
                ok = ok_raw and (passes is None or passes[k])
            if ok:
                C.append(k)
        # ---- rule F: the walk
        kept, V, nxt = sample(C, s, K, N)
        start[i], visited[i], n_fit[i] = s, V, len(kept)
        tot = {k: score_node(op.nodes[k], req, weights) for k in C}
        at = -1
        if kept:
            top = max(tot[k] for _, k in kept)
            at = next(k for _, k in kept if tot[k] == top)                     # the smallest visit position among the maxima
            total[i] = top
            full_top = max(tot.values())
            full_at = min(k for k in C if tot[k] == full_top)
            hz["a"] += int(at != full_at)
            hz["b"] += int(at != min(k for _, k in kept if tot[k] == top))
            hz["l"] += int(sp and own != NOM_NONE and at != full_at)
        if nxt is not None:
            (vk, kk), (vn, kn) = kept[-1], nxt
            hz["c"] += int(slot(s, kk, N) == slot(s, kn, N))
            hz["d"] += int(slot(s, kn, N) >= WAVES)
            hz["x"] += int(slot(s, kk, N) // WAVES < slot(s, kn, N) // WAVES)
            hz["e"] += int(kn < s)
            hz["f"] += int(kn < s and (kn >> 6) == (s >> 6))
            hz["g"] += int(vn - vk > 1)
        hz["h"] += int(K < N and len(C) == K)
        hz["i"] += int(K < N and len(C) < K)
        if sp:
            hz["k"] += int(sample(raw, s, K, N)[1] != V)
        if run_filter:
            unfiltered = sample(raw, s, K, N)[0]
            hz["m"] += int(len(unfiltered) == K and unfiltered[-1][1] not in C)
        s = (s + V) % N if N else 0
        if at < 0:
            continue
        # ---- assume (the pod's own request only), consume (D6), Permit, release: the parent models'
        sor.assume(op.nodes[at], req)
        assumed[i] = at
        if sp and own != NOM_NONE:
            gone = [o for o in live if o.id == own]
            assert len(gone) == 1, "an own id names one live nominee"
            live.remove(gone[0])
            dead.append(gone[0])
            consumed.append((own, i, at))
        if pod.group is None:
            assert op.permit(pod, pod.uid, at) == (True, 2)
            out["pod_node"][i] = at
            continue
        ready, pcode = op.permit(pod, pod.uid, at)
        if not ready:
            continue
        allowed = op.start_batch(pod.group)
        if not allowed:
            continue
        for uid, node in allowed:
            op.postbind(pod.group)
            if uid in uid_index:
                out["pod_node"][uid_index[uid]] = node
        g = gnames.index(pod.group)
        if g in slot_of:
            out["released_pods"][slot_of[g]] += len(allowed)
        else:
            slot_of[g] = len(out["released_group"])
            out["released_group"].append(g)
            out["released_pods"].append(len(allowed))
    op._refresh()
    out["matched"] = [op.cache[nm].matched for nm in gnames]
    out["status_scheduled"] = [nv.u32(op.cache[nm].pod_group.status_scheduled) for nm in gnames]
    out["latch"] = [bool(op.cache[nm].scheduled) for nm in gnames]
    out["closed"] = [op.cache[nm].phase not in (ns.PENDING, ns.PRESCHEDULING, ns.SCHEDULING) for nm in gnames]
    out["denied"] = [op.last_denied.get(nm, op.now) is not None for nm in gnames]
    out["op"] = op
    out["total"], out["n_fit"], out["assumed"] = total, n_fit, assumed
    out["start"], out["visited"], out["next_start"] = start, visited, s
    out["nominees"] = live
    out["consumed"] = sorted(consumed)
    out["hazards"] = hz
    return out
