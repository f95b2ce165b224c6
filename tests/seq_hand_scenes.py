"""The hand-derived scenes of tests/golden/seq_hand_kats.json (TEST INFRASTRUCTURE): loader (shorthands expanded, unknown fields refused), the
scene as naive_ref objects and as SoA through nv.to_soa, the expected record in the shape tests/test_gpu_seq.check_pass compares against,
and `hazards`: the bookkeeping conditions of bs_seq_pass.inc (the registers of the current gang and of the leader, the LDS wait list of 512
entries, the pass-local chain, the 64-pod staging window, the 64-node tiles, the release-record cap) restated over the queue and the expected
record, so that a scene can be held to the device path it is meant to reach.  Nothing here reads kernel text or runs the oracle."""
import copy
import json
import os

import numpy as np

import naive_ref as nv

soa = nv.soa
GI = 1 << 30
KATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seq_hand_kats.json")
WAIT_LIST, POD_WIN, TILE, KEYS_LDS = 512, 64, 64, 8192            # kSeqWaitList, kSeqPodWin, the first-fit tile, the LDS key window
COUNTERS = ("list_valid", "chain_walked", "list_overflowed", "switched_with_waiting", "leader_copy", "window_crossed", "tile_crossed", "cap_exceeded")
STRUCTURAL = ("keys_global", "lanes_run_time", "second_release")  # hazards a scene reaches by its shape (G > 8192, S > 4) or by a second record
# second_release (the has_rec branch: a gang released twice in one pass) is reachable through the ABI only by uint32 wrap: a release needs
# matched >= MinMember - Scheduled (core.go:303) and adds matched to Scheduled (:327), so without wrap Scheduled >= MinMember afterwards and the
# phase closes (:329); the phase stays open only if Scheduled + matched wraps past 2^32 with Scheduled <= MinMember, i.e. matched of about 2^32 on
# entry.  The scene of that name does this; for the same reason there is no scene "one below MinMember after a release".
SCENE_FIELDS = {"name", "kind", "cites", "why", "hazard", "nodes", "groups", "pods", "expect", "passes", "scalars", "n_classes", "stages", "cap", "variants",
                "models", "cpu_only", "steps"}
STEP_FIELDS = {"t", "op", "uid", "pod_name", "group", "req", "node", "expect"}
CPU_ONLY_MAX = 4                                                   # scenes that need a clock or pod UIDs: oracle/naive_seq.SeqOperation only
NODE_FIELDS = {"alloc", "req", "unschedulable", "no_fit", "repeat", "full"}
GROUP_FIELDS = {"name", "min_member", "scheduled", "matched", "closed", "denied", "latch", "min_resources", "rep", "repeat"}
POD_FIELDS = {"group", "req", "cls", "repeat"}
EXPECT_FIELDS = {"pf_code", "pf_first_k", "pf_leader", "expect_node", "pod_node", "released_group", "released_pods", "groups", "requested", "last_permitted",
                 "release_at"}
PASS_FIELDS = {"pods", "expect", "carry_leader"}
GROUP_STATE = {"matched", "status_scheduled", "latch", "closed", "denied"}
FULL = {"alloc": {"cpu": 4000, "memory": 64 * GI, "pods": 10}, "req": {"cpu": 4000}}
FIRST_K = {"ns": soa.K_NOT_SCANNED, "none": soa.K_NONE}


def _known(d, fields, what):
    assert set(d) <= fields, f"{what}: unknown fields {sorted(set(d) - fields)}"


def _expand(entries, fields, what):
    out = []
    for e in entries:
        _known(e, fields, what)
        if "full" in e:
            assert set(e) == {"full"}, what
            out += [FULL] * e["full"]
        elif "repeat" in e:
            body = {k: v for k, v in e.items() if k != "repeat"}
            for j in range(e["repeat"]):
                one = dict(body)
                if "name" in one:
                    one["name"] = one["name"].format(len(out))
                out.append(one)
        else:
            out.append(e)
    return out


def load():
    """the scenes, shorthands expanded, every scene with a list of passes"""
    scenes = []
    for k in json.load(open(KATS))["scenes"]:
        _known(k, SCENE_FIELDS, k.get("name"))
        for f in ("name", "kind", "cites", "why", "hazard"):
            assert isinstance(k[f], str) and k[f], f"{k.get('name')}: {f}"
        assert k["kind"] in ("A", "B") and k["hazard"] in COUNTERS + STRUCTURAL + ("none",), k["name"]
        named = {g["name"] for g in k["groups"] if "repeat" not in g}
        k = dict(k, nodes=_expand(k["nodes"], NODE_FIELDS, k["name"]), groups=_expand(k["groups"], GROUP_FIELDS, k["name"]))
        if k.get("cpu_only"):
            assert isinstance(k["cpu_only"], str) and k["steps"] and "pods" not in k and "passes" not in k, f"{k['name']}: the reason and the steps"
            for st in k["steps"]:
                _known(st, STEP_FIELDS, k["name"])
                assert st["op"] in ("permit", "prefilter", "filter"), k["name"]
            k["passes"] = []
            scenes.append(k)
            continue
        assert "steps" not in k, k["name"]
        passes = k.pop("passes", None) or [dict(pods=k.pop("pods"), expect=k.pop("expect"))]
        assert "pods" not in k and "expect" not in k, k["name"]
        for ps in passes:
            _known(ps, PASS_FIELDS, k["name"])
            _known(ps["expect"], EXPECT_FIELDS, k["name"])
            ps["pods"] = _expand(ps["pods"], POD_FIELDS, k["name"])
            e, p = ps["expect"], len(ps["pods"])
            assert all(len(e[f]) == p for f in ("pf_code", "pf_first_k", "pf_leader", "expect_node", "pod_node")), f"{k['name']}: one answer per pod"
            assert len(e["released_group"]) == len(e["released_pods"]) and set(e["groups"]) == named, f"{k['name']}: every named group has its state"
            assert all(set(v) == GROUP_STATE for v in e["groups"].values()), k["name"]
        k["passes"] = passes
        scenes.append(k)
    assert len({k["name"] for k in scenes}) == len(scenes)
    return scenes


def stages_of(k):
    st = k.get("stages", "prefilter")
    assert st in ("prefilter", "filter_deny")
    return soa.STAGE_PREFILTER | (soa.STAGE_FILTER | soa.BATCH_FILTER_DENY if st == "filter_deny" else 0)


def objects(k, ps_idx=0):
    """pass `ps_idx` of the scene as naive_ref objects: (sc, closed).  The entry state of a later pass is the hand answer of the one before."""
    names = list(k.get("scalars", []))
    nodes = []
    for nd in k["nodes"]:
        a, r = nv.Resource(), nv.Resource()
        a.Add(nd["alloc"])
        r.Add(nd.get("req", {}))
        nodes.append(nv.NodeInfo(a, r, 0, unschedulable=bool(nd.get("unschedulable", False)), labels_fit={int(c): False for c in nd.get("no_fit", [])}))
    cache, closed, denied = {}, set(), set()
    for g in k["groups"]:
        mr = g.get("min_resources")
        pgs = nv.PGS(nv.PodGroup(g["name"], g["min_member"], g.get("scheduled", 0), None if mr is None else dict(mr)), matched=g.get("matched", 0),
                     scheduled=bool(g.get("latch", False)))
        if "rep" in g:
            pgs.pod = nv.Pod(g["name"] + "-rep", g["name"], dict(g["rep"]))
        cache[g["name"]] = pgs
        if g.get("closed"):
            closed.add(g["name"])
        if g.get("denied"):
            denied.add(g["name"])
    for ps in k["passes"][:ps_idx]:                              # the passes before: their hand answers are this pass's entry state
        for nm, st in ps["expect"]["groups"].items():
            pgs = cache[nm]
            pgs.matched, pgs.pod_group.status_scheduled, pgs.scheduled = st["matched"], st["status_scheduled"], st["latch"]
            (closed.add if st["closed"] else closed.discard)(nm)
            (denied.add if st["denied"] else denied.discard)(nm)
        for idx, lanes in ps["expect"]["requested"].items():
            r = nv.Resource()
            r.Add(lanes)
            nodes[int(idx)].requested = r
    queue = k["passes"][ps_idx]["pods"] if k["passes"] else []
    pods = [nv.Pod(f"p{ps_idx}-{i}", p.get("group"), dict(p["req"]), cls=int(p.get("cls", 0))) for i, p in enumerate(queue)]
    sc = dict(nodes=nodes, cache=cache, pods=pods, names=names, n_classes=int(k.get("n_classes", 1)), denied=denied, permitted=set())
    return sc, closed


def to_soa(k, ps_idx=0):
    """(nodes, fit, groups, pods) of pass `ps_idx`: what the device is loaded with"""
    sc, closed = objects(k, ps_idx)
    nodes, fit, groups, pods, gidx = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], denied=sc["denied"], permitted=sc["permitted"])
    for nm in closed:
        groups.flags[gidx[nm]] |= soa.GROUP_PHASE_CLOSED
    return nodes, fit, groups, pods


def expected(k, ps_idx=0, device=False):
    """the hand record of pass `ps_idx` in the shape check_pass takes: the oracle's dict, made of the JSON and the entry state alone.  device: the
    release arrays as a call with the scene's cap returns them (the first cap gangs; n_released counts them all)"""
    nodes, fit, groups, pods = to_soa(k, ps_idx)
    e = k["passes"][ps_idx]["expect"]
    names = list(k.get("scalars", []))
    lane = {"cpu": 0, "memory": 1, "ephemeral-storage": 2, "pods": 3, **{nm: 4 + s for s, nm in enumerate(names)}}
    nodes = nodes.copy()
    for idx, lanes in e["requested"].items():
        for nm, v in lanes.items():
            nodes.requested[lane[nm], int(idx)] = v
            if lane[nm] >= 4:
                nodes.requested_present[int(idx)] |= np.uint32(1 << (lane[nm] - 4))
    groups = copy.deepcopy(groups)
    gidx = {g["name"]: i for i, g in enumerate(k["groups"])}
    for nm, st in e["groups"].items():
        i = gidx[nm]
        groups.matched[i], groups.status_scheduled[i] = st["matched"], st["status_scheduled"]
        f = int(groups.flags[i]) & ~(soa.GROUP_SCHEDULED_LATCH | soa.GROUP_PHASE_CLOSED | soa.GROUP_DENIED)
        groups.flags[i] = f | (soa.GROUP_SCHEDULED_LATCH if st["latch"] else 0) | (soa.GROUP_PHASE_CLOSED if st["closed"] else 0) | (soa.GROUP_DENIED if st["denied"] else 0)
    cap = k.get("cap") if device else None
    rg, rp = e["released_group"], e["released_pods"]
    n = len(rg)
    if cap is not None:
        rg, rp = rg[:cap], rp[:cap]
    p = pods.p
    return dict(pf_code=np.array(e["pf_code"], np.uint8), pf_first_k=np.array([FIRST_K.get(v, v) for v in e["pf_first_k"]], np.uint32),
                pf_leader=np.array(e["pf_leader"], np.int32), pod_node=np.array(e["pod_node"], np.int32), assumed=np.array(e["expect_node"], np.int32),
                released_group=np.array(rg, np.uint32), released_pods=np.array(rp, np.uint32), n_released=n, nodes=nodes, groups=groups,
                stages=stages_of(k), last_permitted=np.array(e.get("last_permitted", [0] * p), np.uint8))


def hazards(k, ps_idx=0) -> dict:
    """the counters of COUNTERS (+ second_release) for one pass, from the queue and the expected record.  The state mirrored: the group in the
    `own` registers and the one in the leader's, the wait list's count and validity, per group the pass-local waiting pods and whether it was
    released before in this pass, the stale leader between calls."""
    nodes, fit, groups, pods = to_soa(k, ps_idx)
    ps = k["passes"][ps_idx]
    e = ps["expect"]
    G, cap = groups.g, k.get("cap")
    cap = G if cap is None else cap
    gidx = {g["name"]: i for i, g in enumerate(k["groups"])}
    last = {}
    for i, p in enumerate(ps["pods"]):
        if e["pod_node"][i] >= 0 and p.get("group") in gidx:
            last[p["group"]] = i
    release_at = set(e.get("release_at", last.values()))
    c = dict.fromkeys(COUNTERS + ("second_release",), 0)
    own_of = ldr_of = -1
    wl_cnt, wl_ok = 0, True
    waiting, has_rec, n_released = {}, set(), 0
    sop = int(ps.get("carry_leader", -1))
    for i, p in enumerate(ps["pods"]):
        gi = gidx.get(p.get("group"), -1)
        grouped = gi >= 0
        miss_own = grouped and gi != own_of
        miss_ldr = sop >= 0 and sop != gi and sop != ldr_of
        if miss_own:
            c["leader_copy"] += int(gi == ldr_of)
            c["switched_with_waiting"] += int(bool(waiting.get(gi)))
            own_of, wl_cnt, wl_ok = gi, 0, not waiting.get(gi)
        if miss_ldr:
            ldr_of = sop
        sop = e["pf_leader"][i]
        at = e["expect_node"][i]
        if at < 0 or not grouped:
            continue
        if i not in release_at:
            waiting.setdefault(gi, []).append(i)
            if wl_cnt < WAIT_LIST:
                wl_cnt += 1
            else:
                wl_ok = False
                c["list_overflowed"] += 1
            continue
        mine = waiting.pop(gi, [])
        if mine:
            from_list = wl_ok and wl_cnt == len(mine)
            c["list_valid" if from_list else "chain_walked"] += 1
        members = mine + [i]
        c["window_crossed"] += int(min(members) // POD_WIN != max(members) // POD_WIN)
        c["tile_crossed"] += int(len({e["expect_node"][m] // TILE for m in members}) > 1)
        if gi in has_rec:
            c["second_release"] += 1
        else:
            c["cap_exceeded"] += int(n_released >= cap)
            n_released += 1
            has_rec.add(gi)
        wl_cnt, wl_ok = 0, True
    c["keys_global"] = int(G > KEYS_LDS)
    c["lanes_run_time"] = int(nodes.lanes - 4 > 4)
    return c
