"""Object-level model of bs_seq_run_scored_nominated (TEST INFRASTRUCTURE): rule SP of include/bsched.h.  The loop of
tests/seq_nominated_ref.replay — nominated pods as objects, added to a deep copy of the node before the fit test (rule S), deleted on the
spot when their pod is assumed (D6) — written out again with tests/seq_scored_ref.total_of in the choice: the pod takes the candidate with
the largest total, ties to the lowest index, and the total is computed from the node ITSELF, never from the copy that holds the nominees
(D8: addNominatedPods works on a copy inside podFitsOnNode, PrioritizeNodes reads the snapshot).  PreFilter never sees a nominee (S1)."""
import naive_ref as nv
import naive_seq as ns
import seq_obj_replay as sor
from seq_nominated_ref import NOM_NONE, Nominee, end_state_soa, objects_to_rows, rows_to_objects, with_rows  # noqa: F401  (the same objects and conversions)
from seq_scored_ref import WEIGHT_MAX, node_lanes, score_node, total_of

HAZARDS = "abcdefghjk"          # the issue's list (it has no letter i)
EXTRA = "si"                    # s: a row's SCALAR lane turns a node away that the row's first four lanes leave open; i: a row brings a scalar key
                                # the node's requests lack into a test that asks for it (the key-present rule decides with the row's lane alone)
WILD = 1 << 40


def _first4(o: Nominee) -> Nominee:
    return Nominee(o.id, o.node, o.priority, nv.Resource(o.req.MilliCPU, o.req.Memory, o.req.EphemeralStorage, 1, None))


def replay(sc, nominees, priority, own_id, weights, closed=(), scalar_names=()):
    """-> seq_obj_replay.replay's dict plus total [p], n_fit [p], assumed [p], nominees (the surviving objects, table order), consumed
    ([(id, queue index, node)] ascending id) and hazards, a count per letter:
    a: the winner differs from the scored choice without a table on the same state (a row turned the maximum away); b: the winner differs
    from the nominated first fit (C's first member); c: the pod's own row sits on the winner and would have turned the pod away had it not been
    left out; d: a row consumed earlier in the pass would have turned the pod (of priority <= the row's) away from the winner; e: a row of EQUAL
    priority blocks a node; f: rows of LOWER priority on the winner would have turned the pod away; g: a node in front of the winner reaches the
    same total and is blocked by a row — the tie goes to the higher index; h: |C| differs from the table-less candidate count; j: the winner
    holds rows the pod sees, and ranking by requests + rows would have chosen another node (D8); k: a row with a cpu or memory lane that is
    negative or >= 2^40 sits on a candidate (the kernel's wild tiles)."""
    assert all(0 <= w <= WEIGHT_MAX for w in weights) and len(weights) == 3
    op = sor.build_operation(sc, closed)
    gnames = list(op.cache.keys())
    uid_index = {pod.uid: i for i, pod in enumerate(sc["pods"])}
    P = len(sc["pods"])
    live, dead = list(nominees), []
    out = dict(pf_code=[], pf_first_k=[], pf_leader=[], pod_node=[-1] * P, released_group=[], released_pods=[], last_permitted=[0] * P)
    total, n_fit, assumed, consumed = [0] * P, [0] * P, [-1] * P, []
    hz = {c: 0 for c in HAZARDS + EXTRA}
    slot_of = {}
    for i, pod in enumerate(sc["pods"]):
        code, fk = op.prefilter(pod)
        out["pf_code"].append(code)
        out["pf_first_k"].append(fk)
        out["pf_leader"].append(gnames.index(op.max_finished_pg) if op.max_pg_status is not None else -1)
        own = NOM_NONE if own_id is None else int(own_id[i])
        if code >= 16:
            continue
        if pod.group is not None and pod.group not in op.cache:
            assert op.permit(pod, pod.uid, 0) == (False, 3)
            continue
        req = nv.pod_resource_require(pod, True)
        req.ScalarResources = {k: v for k, v in (req.ScalarResources or {}).items() if k in scalar_names} or None
        P_i = int(priority[i])
        # ---- the candidates: rule S's test on a copy with the nominees; and, for the census, the raw test
        C, raw, mine_on, seen_on = [], [], {}, {}
        for k, info in enumerate(op.nodes):
            if info.nil or not info.has_node or info.unschedulable or info.taint_err or not nv.check_fit(pod, info):
                continue
            on_k = [o for o in live if o.node == k and o.id != own]
            mine = [o for o in on_k if o.priority >= P_i]
            seen = with_rows(info, mine)
            ok, ok_raw = sor.holds(seen, req), sor.holds(info, req)
            if ok_raw:
                raw.append(k)
            if ok:
                C.append(k)
                mine_on[k], seen_on[k] = mine, seen
            elif ok_raw:
                hz["e"] += int(sor.holds(with_rows(info, [o for o in mine if o.priority > P_i]), req))
                hz["s"] += int(sor.holds(with_rows(info, [_first4(o) for o in mine]), req))
                hz["i"] += int(any(nm not in (info.requested.ScalarResources or {}) and (req.ScalarResources or {}).get(nm, 0) > 0
                                   for o in mine for nm in (o.req.ScalarResources or {})))
        n_fit[i] = len(C)
        hz["h"] += int(len(C) != len(raw))
        # ---- the choice: the largest total over the node's OWN lanes (D8), the lowest index among equals
        tot = {k: score_node(op.nodes[k], req, weights) for k in set(C) | set(raw)}
        top_raw = max((tot[k] for k in raw), default=0)
        at_raw = min((k for k in raw if tot[k] == top_raw), default=-1)
        if not C:
            hz["a"] += int(at_raw >= 0)
            continue
        top = max(tot[k] for k in C)
        at = min(k for k in C if tot[k] == top)
        total[i] = top
        hz["a"] += int(at != at_raw)
        hz["b"] += int(at != C[0])
        hz["g"] += int(any(k < at and tot[k] == top for k in raw if k not in C))
        info = op.nodes[at]
        hz["c"] += int(any(o.node == at and o.id == own and not sor.holds(with_rows(seen_on[at], [o]), req) for o in live))
        hz["d"] += int(any(o.node == at and o.priority >= P_i and not sor.holds(with_rows(seen_on[at], [o]), req) for o in dead))
        low = [o for o in live if o.node == at and o.id != own and o.priority < P_i]
        hz["f"] += int(bool(low) and not sor.holds(with_rows(seen_on[at], low), req))
        if mine_on[at]:
            alt = {k: total_of(*node_lanes(seen_on[k], req), weights) for k in C}
            hz["j"] += int(min(k for k in C if alt[k] == max(alt.values())) != at)
        hz["k"] += int(any(o.node in seen_on and (not 0 <= o.req.MilliCPU < WILD or not 0 <= o.req.Memory < WILD) for o in live))
        # ---- assume (the pod's own request only), consume (D6), Permit, release
        sor.assume(info, req)
        assumed[i] = at
        if own != NOM_NONE:
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
    out["nominees"] = live
    out["consumed"] = sorted(consumed)
    out["hazards"] = hz
    return out
