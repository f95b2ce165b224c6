"""Two statements of bs_seq_expire — a gang's Permit timeout after a sequential pass (TEST INFRASTRUCTURE).

What the reference does when a gang's PodNameUIDs entry runs out: OnEvicted rejects every entry of MatchedPodNodes
(controller.go:322-331 -> batchscheduler.go:346-352), the framework unreserves each pod and the cache forgets it (NodeInfo.RemovePod),
the entries are deleted (controller.go:328), the group goes onto the deny list (controller.go:332 -> core.go:422-425).

* object level: on the SeqOperation tests/seq_obj_replay.replay returns (`out["op"]`): for every live MatchedPodNodes entry un-assume
  the pod on its node (the inverse of seq_obj_replay.assume), delete the entry, optionally add the group to last_denied.
* array level: numpy on the SoA scene.  Where the waiting pods sit is RE-DERIVED by replaying first fit and assume in plain Python from
  the C oracle's pf_code and the holds() rule as include/bsched.h states it; the replay must reproduce the oracle's pod_node for the
  released pods and its node requests after the pass (asserted: the restatement is itself pinned).  PREFILTER-only passes."""
import numpy as np

import naive_ref as nv
import seq_obj_replay as sor

M64 = (1 << 64) - 1
DENIED = 0x08          # BS_GROUP_DENIED


def w64(v: int) -> int:
    """int64 wrap-around"""
    v &= M64
    return v - (1 << 64) if v >> 63 else v


# ---- array level ---------------------------------------------------------------------------------------------------------------------
def _holds(alloc, req, apres, rpres, k, r, pres, S):
    """bsched.h, bs_seq_run: lane j in {cpu, mem, eph} binds when the pod asks for it; pods lane: requested + 1 <= allocatable; a requested
    scalar needs the allocatable key"""
    for j in range(3):
        if r[j] > 0 and r[j] > w64(int(alloc[j, k]) - int(req[j, k])):
            return False
    if int(req[3, k]) + 1 > int(alloc[3, k]):
        return False
    for s in range(S):
        if not (pres >> s) & 1 or r[4 + s] <= 0:
            continue
        if not (int(apres[k]) >> s) & 1:
            return False
        have = int(req[4 + s, k]) if (int(rpres[k]) >> s) & 1 else 0
        if r[4 + s] > int(alloc[4 + s, k]) - have:
            return False
    return True


def waiting_after_pass(nodes, fit, groups, pods, s):
    """-> (wait_node [p] int32: the node a pod still waits on after the pass the oracle recorded in `s`, else -1; created: set of
    (pod, scalar) whose assume step created the node's key).  Asserts that the replay reproduces the oracle."""
    S, N, G, P = nodes.lanes - 4, nodes.n, groups.g, pods.p
    req, rpres = nodes.requested.copy(), nodes.requested_present.copy()
    fitb = fit.to_bool()
    assumed = np.full(P, -1, np.int64)
    created = set()
    for i in range(P):
        if s["pf_code"][i] >= 16:
            continue
        gi = int(pods.group[i])
        grouped = 0 <= gi < G
        if gi != -1 and not grouped:
            continue
        r = [int(pods.req[j, i]) for j in range(nodes.lanes)]
        pres, cls = int(pods.req_present[i]), int(pods.cls[i])
        at = -1
        for k in range(N):
            if nodes.flags[k] or cls >= fit.n_classes or not fitb[cls, k]:
                continue
            if _holds(nodes.allocatable, req, nodes.allocatable_present, rpres, k, r, pres, S):
                at = k
                break
        if at < 0:
            continue
        for j in range(3):
            req[j, at] = w64(int(req[j, at]) + r[j])
        req[3, at] = w64(int(req[3, at]) + 1)
        for sc in range(S):
            if (pres >> sc) & 1:
                if not (int(rpres[at]) >> sc) & 1:
                    req[4 + sc, at] = 0
                    created.add((i, sc))
                req[4 + sc, at] = w64(int(req[4 + sc, at]) + r[4 + sc])
                rpres[at] |= np.uint32(1 << sc)
        assumed[i] = at
    rel = s["pod_node"] >= 0
    assert np.array_equal(assumed[rel], s["pod_node"][rel]), "replay: the released pods' nodes"
    assert np.array_equal(req, s["nodes"].requested) and np.array_equal(rpres, s["nodes"].requested_present), "replay: node requests after the pass"
    grouped = (pods.group >= 0) & (pods.group < G)
    wait = np.where(grouped & (assumed >= 0) & ~rel, assumed, -1).astype(np.int32)
    return wait, created


class State:
    """what bs_seq_expire works on: node requests + keys, group matched + flags, the waiting pods' nodes"""

    def __init__(self, requested, requested_present, matched, flags, wait_node):
        self.requested, self.requested_present = requested.copy(), requested_present.copy()
        self.matched, self.flags, self.wait_node = matched.copy(), flags.copy(), wait_node.copy()

    @staticmethod
    def after_pass(nodes, fit, groups, pods, s):
        wait, _ = waiting_after_pass(nodes, fit, groups, pods, s)
        return State(s["nodes"].requested, s["nodes"].requested_present, s["groups"].matched, s["groups"].flags, wait)

    def copy(self):
        return State(self.requested, self.requested_present, self.matched, self.flags, self.wait_node)


def expire(st: State, pods, groups=None, deny=False, all=False):
    """bs_seq_expire on `st` (mutated).  -> dict of the call's full results (no caps)"""
    S = st.requested.shape[0] - 4
    chains = {}
    for i in np.nonzero(st.wait_node >= 0)[0]:
        chains.setdefault(int(pods.group[i]), []).append(int(i))
    glist = sorted(chains) if all else [int(g) for g in groups]
    out = dict(group=[], group_pods=[], group_earlier=[], pod=[], node=[])
    for g in glist:
        mine = chains.get(g, [])                                  # ascending queue index
        for i in mine:
            k = int(st.wait_node[i])
            pres = int(pods.req_present[i])
            for j in range(3):
                st.requested[j, k] = w64(int(st.requested[j, k]) - int(pods.req[j, i]))
            st.requested[3, k] = w64(int(st.requested[3, k]) - 1)
            for sc in range(S):
                if (pres >> sc) & 1:                              # the lane loses the request, its node bit stays
                    if not (int(st.requested_present[k]) >> sc) & 1:     # (a key the node lost since the pass: 0 before, the bit set)
                        st.requested[4 + sc, k] = 0
                        st.requested_present[k] |= np.uint32(1 << sc)
                    st.requested[4 + sc, k] = w64(int(st.requested[4 + sc, k]) - int(pods.req[4 + sc, i]))
            out["pod"].append(i)
            out["node"].append(k)
            st.wait_node[i] = -1
        out["group"].append(g)
        out["group_pods"].append(len(mine))
        out["group_earlier"].append((int(st.matched[g]) - len(mine)) & 0xFFFFFFFF)
        st.matched[g] = 0
        if deny:
            st.flags[g] |= np.uint8(DENIED)
    res = {k: np.array(v, np.uint32) for k, v in out.items()}
    res["n_groups"], res["n_pods"] = len(out["group"]), len(out["pod"])
    return res


# ---- object level --------------------------------------------------------------------------------------------------------------------
def unassume(info, req: nv.Resource):
    """the inverse of seq_obj_replay.assume (NodeInfo.RemovePod): a scalar key stays in the map"""
    r = info.requested
    r.MilliCPU -= req.MilliCPU
    r.Memory -= req.Memory
    r.EphemeralStorage -= req.EphemeralStorage
    if r.AllowedPodNumber:
        r.AllowedPodNumber -= 1
    else:
        info.pod_count -= 1
    for name, want in (req.ScalarResources or {}).items():
        r.ScalarResources[name] = r.ScalarResources.get(name, 0) - want


def expire_objects(op, sc, names, deny=False, scalar_names=()):
    """OnEvicted for the groups `names` on the SeqOperation a replay left.  -> per group (pods of the pass as (queue index, node)
    ascending, entries without a queue index)"""
    by_uid = {pod.uid: (i, pod) for i, pod in enumerate(sc["pods"])}
    out = []
    for nm in names:
        g = op.cache[nm]
        rows, earlier = [], 0
        for uid, (node, _) in sorted(g.matched_pod_nodes.live(op.now).items()):
            if uid in by_uid:
                i, pod = by_uid[uid]
                req = nv.pod_resource_require(pod, True)
                req.ScalarResources = {k: v for k, v in (req.ScalarResources or {}).items() if k in scalar_names} or None
                unassume(op.nodes[node], req)                     # waitingPod.Reject -> unreserve -> the cache forgets the pod
                rows.append((i, node))
            else:
                earlier += 1                                      # an earlier cycle's waiting pod: the caller's to take off its node
            g.matched_pod_nodes.delete(uid)                       # controller.go:328
        if deny:
            op.last_denied.add(nm, "", op.now, 20 * 1_000_000_000)   # controller.go:332 -> core.go:422-425
        out.append((sorted(rows), earlier))
    op._refresh()
    return out


def object_nodes_soa(op, sc):
    return nv.to_soa(op.nodes, {}, [], sc["names"], sc["n_classes"])[0]
