"""Object-level model of bs_seq_run_scored (TEST INFRASTRUCTURE): the loop of tests/seq_obj_replay.replay written out again with rule P (D7) of
include/bsched.h in the node choice.  For every pod the set C of nodes the node rule accepts is collected in list order (flags, checkFit,
[the plugin's Filter], holds); the scored pass takes the member of C with the largest total, ties to the lowest index, where the plain pass
takes C's first member.  score_node is a scalar statement of the rule on Python ints and floats (binary64, one rounding per operation);
everything around the choice is the plain replay's.  The end state is converted to the SoA the GPU tests compare."""
import naive_ref as nv
import naive_seq as ns
import seq_obj_replay as sor
from seq_nominated_ref import end_state_soa          # noqa: F401  (the same conversion: the model's dict has the keys it reads)

WEIGHT_MAX = 65536
DOMAIN = 1 << 53
HAZARDS = "abcdefghi"


def in_domain(A: int, R: int) -> bool:
    return 0 < A < DOMAIN and 0 <= R <= A


def lane_parts(A: int, R: int):
    """(least_j, most_j, frac_j) of one lane"""
    if not in_domain(A, R):
        return 0, 0, 1.0
    return ((A - R) * 100) // A, (R * 100) // A, float(R) / float(A)      # (nothing is negative in the domain: // truncates)


def parts(A0: int, R0: int, A1: int, R1: int):
    """(least, most, balanced) of a node from its two scoring lanes"""
    l0, m0, f0 = lane_parts(A0, R0)
    l1, m1, f1 = lane_parts(A1, R1)
    balanced = 0 if f0 >= 1.0 or f1 >= 1.0 else int((1.0 - abs(f0 - f1)) * 100.0)
    return (l0 + l1) // 2, (m0 + m1) // 2, balanced


def total_of(A0, R0, A1, R1, weights) -> int:
    least, most, balanced = parts(A0, R0, A1, R1)
    return weights[0] * least + weights[1] * most + weights[2] * balanced


def node_lanes(info, req: nv.Resource):
    """(A0, R0, A1, R1): allocatable and requested + request (wrapping) on the cpu and the memory lane"""
    a, r = info.allocatable, info.requested
    return a.MilliCPU, nv.wrap64(r.MilliCPU + req.MilliCPU), a.Memory, nv.wrap64(r.Memory + req.Memory)


def score_node(info, req: nv.Resource, weights) -> int:
    return total_of(*node_lanes(info, req), weights)


def replay(sc, weights, closed=(), run_filter=False, filter_deny=False, scalar_names=()):
    """-> seq_obj_replay.replay's dict plus total [p], n_fit [p], assumed [p] (the node every pod was assumed on, -1 none) and hazards, a
    count per letter: a: the choice differs from first fit; b: the maximum is shared and the index decides; c: least / most alone would tie
    and balanced decides; d: a candidate has a lane out of domain; e: a pod's pf_code or pf_first_k differs from the first-fit pass on the
    same scene; f: the winner lies in another tile of 64 nodes than the first fit; g: the winner ends at R == A on a lane; h: the winner's
    least_0 + least_1 or most_0 + most_1 is odd and is halved; i: Filter removes the node that would have won."""
    assert all(0 <= w <= WEIGHT_MAX for w in weights) and len(weights) == 3
    op = sor.build_operation(sc, closed)
    gnames = list(op.cache.keys())
    uid_index = {pod.uid: i for i, pod in enumerate(sc["pods"])}
    P = len(sc["pods"])
    out = dict(pf_code=[], pf_first_k=[], pf_leader=[], pod_node=[-1] * P, released_group=[], released_pods=[], last_permitted=[0] * P)
    total, n_fit, assumed = [0] * P, [0] * P, [-1] * P
    hz = {c: 0 for c in HAZARDS}
    slot_of = {}
    for i, pod in enumerate(sc["pods"]):
        code, fk = op.prefilter(pod)
        out["pf_code"].append(code)
        out["pf_first_k"].append(fk)
        out["pf_leader"].append(gnames.index(op.max_finished_pg) if op.max_pg_status is not None else -1)
        if code >= 16:
            continue
        if pod.group is not None and pod.group not in op.cache:
            assert op.permit(pod, pod.uid, 0) == (False, 3)
            continue
        req = nv.pod_resource_require(pod, True)
        req.ScalarResources = {k: v for k, v in (req.ScalarResources or {}).items() if k in scalar_names} or None
        passes = None
        if run_filter:
            passes = []
            for k in range(len(op.nodes)):
                if filter_deny:
                    fl, fn = op.filter(pod, k)
                else:
                    inner = nv.ScheduleOperation(op.nodes, op.cache)
                    inner.max_finished_pg, inner.max_pg_status = op.max_finished_pg, op.max_pg_status
                    fl, fn = inner.filter_node(pod, k)
                passes.append(fl < 16 and (fl != nv.soa.FL_EVALUATED or fn < 16))
            if filter_deny and pod.group is not None:
                out["last_permitted"][i] = int(op.last_permitted.get(pod.uid, op.now) is not None and any(passes))
        # ---- C in list order, with and without the plugin's Filter
        unfiltered = [k for k, info in enumerate(op.nodes)
                      if not (info.nil or not info.has_node or info.unschedulable or info.taint_err or not nv.check_fit(pod, info)) and sor.holds(info, req)]
        C = [k for k in unfiltered if passes is None or passes[k]]
        n_fit[i] = len(C)
        if not C:
            continue
        tot = {k: score_node(op.nodes[k], req, weights) for k in unfiltered}
        top = max(tot[k] for k in C)
        at = min(k for k in C if tot[k] == top)
        total[i] = top
        # ---- the hazards
        lanes = {k: node_lanes(op.nodes[k], req) for k in C}
        hz["a"] += int(at != C[0])
        hz["b"] += int(sum(1 for k in C if tot[k] == top) > 1)
        pr = {k: parts(*lanes[k]) for k in C}
        partial = {k: weights[0] * pr[k][0] + weights[1] * pr[k][1] for k in C}
        rivals = [k for k in C if partial[k] == max(partial.values())]
        hz["c"] += int(weights[2] > 0 and at in rivals and any(pr[k][2] < pr[at][2] for k in rivals))
        hz["d"] += int(any(not in_domain(A0, R0) or not in_domain(A1, R1) for A0, R0, A1, R1 in lanes.values()))
        hz["f"] += int((at >> 6) != (C[0] >> 6))
        A0, R0, A1, R1 = lanes[at]
        hz["g"] += int((in_domain(A0, R0) and R0 == A0) or (in_domain(A1, R1) and R1 == A1))
        l0, m0, _ = lane_parts(A0, R0)
        l1, m1, _ = lane_parts(A1, R1)
        hz["h"] += int((weights[0] > 0 and (l0 + l1) & 1) or (weights[1] > 0 and (m0 + m1) & 1))
        best_unf = max(tot.values())
        hz["i"] += int(min(k for k in unfiltered if tot[k] == best_unf) not in C)
        # ---- assume, Permit, release: the plain replay's
        sor.assume(op.nodes[at], req)
        assumed[i] = at
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
    plain = sor.replay(sc, closed=closed, run_filter=run_filter, filter_deny=filter_deny, scalar_names=scalar_names)
    hz["e"] = sum(1 for i in range(P) if (out["pf_code"][i], out["pf_first_k"][i]) != (plain["pf_code"][i], plain["pf_first_k"][i]))
    out["hazards"] = hz
    return out
