"""Object-level model of bs_seq_run_nominated (TEST INFRASTRUCTURE): the loop of tests/seq_obj_replay.replay written out again with rule S of
include/bsched.h.  Nominated pods are real objects in a list; before the fit test of pod i on node k every nominee on k with priority >= the
pod's, other than the pod's own nomination, is added (NodeInfo.AddPod, wrapping sums) to a DEEP COPY of the node, and `holds` is asked about
the copy — upstream's addNominatedPods inside podFitsOnNode.  PreFilter never sees a nominee (library rule S1: the plugin's cluster sums read
its own NodeInfo).  When a pod that has a nomination is assumed, on whatever node, the nomination object is deleted on the spot (D6:
scheduleOne -> assume -> SchedulingQueue.DeleteNominatedPodIfExists).  The end state is also converted to the SoA the GPU tests compare."""
import copy
from dataclasses import dataclass

import numpy as np

import naive_ref as nv
import naive_seq as ns
import seq_obj_replay as sor

NOM_NONE = 0xFFFFFFFF
HAZARDS = "abcdefghijkl"        # a-j: the issue's list; k, l: two more cursor hazards (see replay)


@dataclass
class Nominee:
    id: int
    node: int
    priority: int
    req: nv.Resource          # as AddPod counts it; the pods lane is 1 by definition


def rows_to_objects(rows: dict | None, scalar_names) -> list:
    """the columns of bs_nominated_read (id, node, priority, req [L][m], req_present) -> Nominee objects in table order"""
    out = []
    if rows is None:
        return out
    for i in range(len(rows["id"])):
        r = nv.Resource(int(rows["req"][0, i]), int(rows["req"][1, i]), int(rows["req"][2, i]), 1, None)
        sc = {nm: int(rows["req"][4 + s, i]) for s, nm in enumerate(scalar_names) if (int(rows["req_present"][i]) >> s) & 1}
        r.ScalarResources = sc or None
        out.append(Nominee(int(rows["id"][i]), int(rows["node"][i]), int(rows["priority"][i]), r))
    return out


def objects_to_rows(objs: list, scalar_names) -> dict:
    m, L = len(objs), 4 + len(scalar_names)
    req, pres = np.zeros((L, m), np.int64), np.zeros(m, np.uint32)
    for i, o in enumerate(objs):
        req[:4, i] = (o.req.MilliCPU, o.req.Memory, o.req.EphemeralStorage, 1)
        for s, nm in enumerate(scalar_names):
            if nm in (o.req.ScalarResources or {}):
                req[4 + s, i] = o.req.ScalarResources[nm]
                pres[i] |= np.uint32(1 << s)
    return dict(id=np.array([o.id for o in objs], np.uint32), node=np.array([o.node for o in objs], np.uint32),
                priority=np.array([o.priority for o in objs], np.int32), req=req, req_present=pres)


def add_pod(info, req: nv.Resource):
    """NodeInfo.AddPod of a nominee on a COPY of the node: every lane, wrapping (rule N's sums)"""
    r = info.requested
    r.MilliCPU = nv.wrap64(r.MilliCPU + req.MilliCPU)
    r.Memory = nv.wrap64(r.Memory + req.Memory)
    r.EphemeralStorage = nv.wrap64(r.EphemeralStorage + req.EphemeralStorage)
    if r.AllowedPodNumber:
        r.AllowedPodNumber += 1
    else:
        info.pod_count += 1
    for name, want in (req.ScalarResources or {}).items():
        if r.ScalarResources is None:
            r.ScalarResources = {}
        r.ScalarResources[name] = nv.wrap64(r.ScalarResources.get(name, 0) + want)


def with_rows(info, rows):
    """a copy of the node with the nominees `rows` added; the node itself when there are none"""
    if not rows:
        return info
    c = copy.deepcopy(info)
    for o in rows:
        add_pod(c, o.req)
    return c


def with_nominees(info, k, nominees, prio, own):
    """the NodeInfo podFitsOnNode tests: a copy with the nominees of node k added (priority >= the pod's, not the pod's own)"""
    return with_rows(info, [o for o in nominees if o.node == k and o.priority >= prio and o.id != own])


def _wraps(info, rows):
    """adding `rows` to the node wraps int64 on the cpu or memory lane"""
    c, m = info.requested.MilliCPU, info.requested.Memory
    for o in rows:
        c, m = c + o.req.MilliCPU, m + o.req.Memory
    return c != nv.wrap64(c) or m != nv.wrap64(m)


def replay(sc, nominees, priority, own_id=None, closed=(), scalar_names=()):
    """-> seq_obj_replay.replay's dict plus nominees (the surviving objects, table order), consumed ([(id, queue index, node)] ascending id)
    blocked (pods for which a nominee turned a node away that would have held them) and hazards, a count per hazard letter of the
    issue's list (a: turned away and placed on a later node; b: a row of EQUAL priority decided; c: a higher-priority pod passed over a row
    that would have turned it away; d: the pod fits only because its own row is left out; e: after a consume a later pod of the same
    request and fit class lands in front of where that class's last search ended — in an EARLIER TILE of 64 nodes, or anywhere after a search
    that found nothing: the granularity of the kernel's cursors; f: the same without a consume in between, after a pod of lower priority;
    k: the same for a pod that has an own row; l: the same although no row was consumed and the earlier pod's priority was not lower — a
    row GREW the room (a negative lane, a sum that wraps) or a pod's negative request freed some; g: a pod with an own row is rejected by PreFilter and keeps it; h: a consumed row whose pod
    is not released by the end of the pass; i: a row brings a scalar the node's requests lack into a test that asks for it; j: a sum wraps)."""
    op = sor.build_operation(sc, closed)
    gnames = list(op.cache.keys())
    uid_index = {pod.uid: i for i, pod in enumerate(sc["pods"])}
    P = len(sc["pods"])
    live = list(nominees)
    out = dict(pf_code=[], pf_first_k=[], pf_leader=[], pod_node=[-1] * P, released_group=[], released_pods=[], last_permitted=[0] * P)
    consumed, blocked, assumed = [], 0, [-1] * P
    hz = {c: 0 for c in HAZARDS}
    last_end = {}                                               # (request, fit class) -> (node its last search ended at, that pod's priority, consumes so far)
    slot_of = {}
    for i, pod in enumerate(sc["pods"]):
        code, fk = op.prefilter(pod)
        out["pf_code"].append(code)
        out["pf_first_k"].append(fk)
        out["pf_leader"].append(gnames.index(op.max_finished_pg) if op.max_pg_status is not None else -1)
        own = NOM_NONE if own_id is None else int(own_id[i])
        if code >= 16:
            hz["g"] += int(own != NOM_NONE)
            continue
        if pod.group is not None and pod.group not in op.cache:
            assert op.permit(pod, pod.uid, 0) == (False, 3)
            continue
        req = nv.pod_resource_require(pod, True)
        req.ScalarResources = {k: v for k, v in (req.ScalarResources or {}).items() if k in scalar_names} or None
        P_i = int(priority[i])
        at, turned = -1, False
        for k, info in enumerate(op.nodes):
            if info.nil or not info.has_node or info.unschedulable or info.taint_err or not nv.check_fit(pod, info):
                continue
            on_k = [o for o in live if o.node == k and o.id != own]
            mine = [o for o in on_k if o.priority >= P_i]
            seen = with_rows(info, mine)
            if mine:
                hz["j"] += int(_wraps(info, mine))
                hz["i"] += int(any(nm not in (info.requested.ScalarResources or {}) and (req.ScalarResources or {}).get(nm, 0) > 0
                                   for o in mine for nm in (o.req.ScalarResources or {})))
            if sor.holds(seen, req):
                at = k
                hz["c"] += int(len(on_k) > len(mine) and not sor.holds(with_rows(info, on_k), req))
                hz["d"] += int(any(o.node == k and o.id == own and not sor.holds(with_rows(seen, [o]), req) for o in live))
                break
            if mine and sor.holds(info, req):
                turned = True
                hz["b"] += int(sor.holds(with_rows(info, [o for o in mine if o.priority > P_i]), req))
        blocked += int(turned)
        hz["a"] += int(turned and at >= 0)
        # the cursor hazards, counted where the kernel can see them: its cursors work on TILES of 64 nodes (a search starts at lane 0 of the
        # tile its class's last search ended in, or is skipped when that search found no node), so a pod is "in front" only when it lands
        # in an earlier tile, or lands at all after a search that found nothing
        key = (repr(sorted(pod.requests.items())), pod.cls)
        if key in last_end and at >= 0:
            end, p_end, n_cons = last_end[key]
            if (at >> 6) < (end >> 6) or end >= len(op.nodes):
                if own != NOM_NONE:
                    hz["k"] += 1
                elif len(consumed) > n_cons:
                    hz["e"] += 1
                elif P_i > p_end:
                    hz["f"] += 1
                else:
                    hz["l"] += 1
        if own == NOM_NONE:
            last_end[key] = (at if at >= 0 else len(op.nodes), P_i, len(consumed))
        if at < 0:
            continue
        sor.assume(op.nodes[at], req)
        assumed[i] = at
        if own != NOM_NONE:                                     # D6: the nomination is deleted with the assume, whatever follows
            gone = [o for o in live if o.id == own]
            assert len(gone) == 1, "an own id names one live nominee"
            live.remove(gone[0])
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
    out["nominees"] = live
    out["consumed"] = sorted(consumed)
    hz["h"] = sum(1 for _, i, _ in consumed if out["pod_node"][i] < 0)
    out["hazards"] = hz
    out["blocked"] = blocked
    out["assumed"] = assumed
    return out


def end_state_soa(out, sc, soa, owner_ids):
    """(Nodes, Groups, wait_node [p]) the model's pass left, as the GPU tests read them back.  owner_ids: the dict the scene's own to_soa call
    filled (owner strings keep their numbers)."""
    op = out["op"]
    names = list(op.cache.keys())
    nodes, _, groups, _, _ = nv.to_soa(op.nodes, op.cache, [], sc["names"], sc["n_classes"], denied={nm for nm, d in zip(names, out["denied"]) if d},
                                       owner_ids=owner_ids)
    for g, c in enumerate(out["closed"]):
        if c:
            groups.flags[g] |= soa.GROUP_PHASE_CLOSED
    groups.status_scheduled[:] = np.array(out["status_scheduled"], np.uint32)
    by_uid = {pod.uid: i for i, pod in enumerate(sc["pods"])}
    wait = np.full(len(sc["pods"]), -1, np.int32)
    for nm in names:
        for uid, (node, _) in op.cache[nm].matched_pod_nodes.live(op.now).items():
            if uid in by_uid:
                wait[by_uid[uid]] = node
    return nodes, groups, wait
