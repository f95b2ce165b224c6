"""Scenes at the int64 extremes (TEST INFRASTRUCTURE) and a CPU classifier that says which pruning guards a query needs.

The reference's running sums (core.go:602,621) and the leader's pre-allocation (core.go:774-793) are Go int64 and wrap (oracle rule
U5).  The device keeps chunk-local sums plus a wrapping chunk offset and prunes 64-row groups with `max(local sums) + offset`; that
bound holds only while nothing wraps, so every chain carries a guard.  The scenes here are built so that a scan WITHOUT the guard
prunes the group that holds the reference's answer.

Construction: one resource lane (cpu, or a scalar key) carries the extreme magnitudes; memory, at ordinary magnitude, decides where
the first covering prefix lies, so the scan has to walk through the extreme groups.  Allocatable quantities are single powers of two
(exact in float32): at pct 1.0 int64(float32(a) * pct) is the identity, at pct 0.7 it is 11744051 * a / 2^24 exactly.  Scenes come
tuned for one of the two percentages (`pct`): the head rows' scaled sum lies just below 2^63 and a few rows BEHIND the answer push the
reference sum over it.  Negative node amounts come from `requested` (never scaled): nodes whose requested far exceeds allocatable.

Everything is built at object level (oracle/naive_ref.py) and marshalled by nv.to_soa, so both oracle statements can run it.
`rows` = 256 (the device's table chunk) for the GPU scenes; a smaller value shrinks the same layout for the naive restatement.
"""
from dataclasses import dataclass, field

import numpy as np

import naive_ref as nv

soa = nv.soa
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
SAFE = 1 << 62
CHUNK, GROUP = 256, 64                      # the device's table chunk and pruning group (bs_common.hpp: kTblChunk, 64-row groups)
SCALARS = ["nvidia.com/gpu", "tencent.cr/tencentip"]
MEM_STEP = 1 << 40                          # the decision lane's step at an answer row
SINGLE_FAMILIES = ("offset-high", "offset-low", "risky-group", "risky-group-low", "wrap-and-return", "wrap-and-return-low",
                   "totals-edge", "far", "far-window", "scalar-lane", "filter-wrap")
BATCH_FAMILIES = ("offset-high", "offset-low", "risky-group", "wrap-and-return", "totals-edge", "scalar-lane", "mixed-tile",
                  "prealloc-wrap", "filter-wrap")
MUST_NEED_A_GUARD = ("offset-high", "offset-low", "risky-group", "wrap-and-return", "far", "far-window", "scalar-lane")


@dataclass
class Scene:
    family: str
    pct: float                               # the percentage the extreme rows are tuned for
    sc: dict                                 # object level: nodes, cache, pods, names, n_classes, denied, permitted
    nodes: object
    fit: object
    groups: object
    pods: object
    queries: list = field(default_factory=list)      # single queries: (cls, pct, request lanes, present mask)
    ext: int = 0                             # the lane that carries the extremes
    answers: tuple = ()                      # rows where the decision lane steps

    @property
    def S(self):
        return len(self.sc["names"])


def _pow2(lo, hi):
    return [1 << k for k in range(lo, hi + 1)]


def _head(pct):
    """allocatable amounts whose scaled sum H lies in [2^62, 2^63): 2^63 - 2^50 at pct 1.0, 0.7f * (2^63 - 2^59) at pct 0.7"""
    return _pow2(50, 62) if pct == 1.0 else _pow2(59, 62)


def _push(pct, count):
    """amounts behind the answer row that take H over 2^63 while the group's LOCAL sums stay below 2^62"""
    return [1 << 51] * count if pct == 1.0 else ([1 << 60] * 4 + [0] * count)[:count]


class _Table:
    """node rows under construction: per row the extreme lane's allocatable / requested and the decision lane's allocatable"""

    def __init__(self, n, scalar=False):
        self.n, self.scalar = n, scalar
        self.alloc, self.req, self.mem = [0] * n, [0] * n, [0] * n
        self.has_key = [True] * n            # scalar scenes: rows whose node carries the extreme key at all
        self.answers = []

    def put(self, at, amounts, neg=False):
        for i, v in enumerate(amounts):
            if neg:
                self.req[at + i] = v
            else:
                self.alloc[at + i] = v
        return at + len(amounts)

    def answer(self, row):
        self.mem[row] = MEM_STEP
        self.answers.append(row)

    def danger_group(self, base, g, pct, neg=False):
        """a 64-row group (g rows in the small layout) whose answer row sits in front of the rows that make the sum wrap"""
        ao = g * 11 // 16
        self.put(base, [1 << 40] * (ao + 1), neg)
        self.put(base + ao + 1, _push(pct, g - ao - 1) if not neg else [1 << 51] * (g - ao - 1), neg)
        self.answer(base + ao)
        return base + ao

    def objects(self):
        out = []
        for i in range(self.n):
            a, r = nv.Resource(), nv.Resource()
            if self.scalar:
                al = {"cpu": 64000, "memory": self.mem[i], "pods": 110, SCALARS[1]: 8}
                rq = {"cpu": 1000, "memory": 0, SCALARS[1]: 2}
                if self.has_key[i]:
                    al[SCALARS[0]], rq[SCALARS[0]] = self.alloc[i], self.req[i]
            else:
                al = {"cpu": self.alloc[i], "memory": self.mem[i], "pods": 110}
                rq = {"cpu": self.req[i], "memory": 0}
            a.Add(al)
            r.Add(rq)
            out.append(nv.NodeInfo(a, r, 1))
        return out


def _table(family, pct, rows):
    """the node rows of a family; `rows` is the chunk size the layout is drawn for"""
    g = rows // 4
    scalar = family == "scalar-lane"
    if family in ("offset-high", "mixed-tile", "prealloc-wrap", "scalar-lane"):
        t = _Table(rows * 2 + 3 * g - 4, scalar)                  # 700 nodes at rows = 256: three chunks, the last one ragged
        first = g + 5 if scalar else 0                            # scalar: the key first appears in the middle of chunk 0 (chunk_kp)
        if scalar:
            t.has_key[:first] = [False] * first
        t.put(first, _head(pct))
        t.danger_group(rows, g, pct)
        t.answer(rows + 2 * g + 3)                                # a second step: behind the wrap, where the extreme sum is negative
    elif family == "offset-low":
        t = _Table(rows * 2 + 3 * g - 4)
        t.put(0, _pow2(50, 62), neg=True)                         # chunk 0 sums to -(2^63 - 2^50)
        t.answer(rows + 3)                                        # in front of the wrap: the extreme sum is hugely negative here
        t.danger_group(rows + g, g, pct, neg=True)                # the sum falls below -2^63 and comes back large and positive
    elif family in ("risky-group", "risky-group-low"):
        neg = family.endswith("low")
        t = _Table(rows * 2 + 3 * g - 4)
        if pct == 1.0 or neg:
            t.put(3, [1 << 41], neg)                              # a small offset, inside (-2^62, 2^62)
            t.put(rows, [1 << 62], neg)                           # the local sum leaves (-2^62, 2^62) at the group's first row
            t.put(rows + 6, _pow2(40, 61)[::-1][: g - 8], neg)    # ... and climbs to within 2^40 of the wrap: max + offset wraps
        else:                                                     # 0.7f * (2^63 * 1.421875) = 0.9953 * 2^63; the offset 0.7f * 2^56 takes it over
            t.put(3, [1 << 56])
            t.put(rows, [1 << 62] * 2)
            t.put(rows + 6, [1 << 61, 1 << 60, 1 << 58, 1 << 57])
        t.answer(rows + 4)
        t.answer(rows + g + 2)
    elif family in ("wrap-and-return", "wrap-and-return-low"):
        neg = family.endswith("low")
        t = _Table(rows * 2 + 3 * g - 4)
        big = [1 << 62] * 2 if (pct == 1.0 or neg) else [1 << 62] * 3
        t.put(0, big, neg)                                        # the reference sum passes +-2^63 inside chunk 0 ...
        t.answer(5)                                               # (a step in front: the sum has the wrong sign here)
        t.put(rows + 2, big, neg)                                 # ... and returns across zero in chunk 1
        t.put(rows + 2 + len(big), [1 << 50] * 2, neg)
        if neg:
            t.put(rows + 5 + len(big), [1 << 61], False)          # low mirror: from below -2^63 up to large positive
        t.answer(rows + g // 2)                                   # the first covering row lies BEHIND the wrap
        t.put(rows + g // 2 + 1, [1 << 62] * 2, neg)              # later rows of the same group wrap again: max + offset is useless
    elif family == "totals-edge":
        t = _Table(rows * 5 + g + 7)                              # chunk totals 0, -1, INT64_MIN, 2^40 (zero low half), then the answer
        t.put(0, [-(1 << 50)], neg=True)                          # (amounts through `requested`: the same totals at every percentage)
        t.put(1, [1 << 50], neg=True)
        t.put(rows, [1], neg=True)
        t.put(2 * rows, [1 << 62] * 2, neg=True)
        t.put(3 * rows + 9, [-(1 << 40)], neg=True)
        t.put(4 * rows, [-(1 << 62)] * 2, neg=True)               # back to 2^40 - 1
        t.answer(4 * rows + 5)
        t.answer(4 * rows + g + 1)
    elif family in ("far", "far-window"):
        if rows == CHUNK:
            t = _Table(8500 if family == "far" else 17000)
            base = 8256 if family == "far" else 16640             # group 129 (fetched from memory) / group 260 in the second window
        else:
            t, base = _Table(rows * 6), rows * 4 + g
        t.put(0, _head(pct))
        t.danger_group(base, g, pct)
        t.answer(base + g + 9)
    elif family == "filter-wrap":
        t = _Table(rows * 2 + 3 * g - 4)
        for at in range(0, t.n, 7):                               # allocatable - requested wraps in both directions (core.go:460-463)
            kind = (at // 7) % 4
            t.alloc[at], t.req[at] = [(1 << 62, -(1 << 62)), (-(1 << 62), (1 << 62) + (1 << 50)), (1 << 62, 0), (0, 1 << 62)][kind]
        t.answer(rows + 3)
        t.answer(rows + g + 5)
    else:
        raise ValueError(family)
    return t


def _single_queries(t, ext, S):
    """a battery per scene: tiny / huge / sentinel requests on the extreme lane x requests on the decision lane x both percentages"""
    out = []
    for pct in (1.0, 0.7):
        for e in (500, 0, -1, 1 << 62, I64_MAX, I64_MIN + 1):
            for m in (1 << 39, 0, 3 << 39, 1 << 42):
                req = [0] * (4 + S)
                req[soa.LANE_MEM], req[soa.LANE_PODS] = m, 1
                req[ext] = e
                if S:
                    req[5] = 3
                    out.append((0, pct, req, 0b11))
                    if e in (500, 0):                             # the pod does not name the extreme key: the `absok` path
                        r2 = list(req)
                        r2[ext] = 0
                        out.append((0, pct, r2, 0b10))
                else:
                    out.append((0, pct, req, 0))
    return out


def _groups_and_pods(family, t, pct, ext, S, n_groups, n_pods, n_classes):
    """gangs and a queue over the scene.  pct 0.7: every gang has its pod and MinResources and the leader has matched pods (the steady
    state: reservation checks, core.go:157-161).  pct 1.0: nobody has matched pods (first checks, core.go:136-147) and every third gang
    still waits for its first pod (captures and MinResources defaults inside the queue)."""
    key = SCALARS[0] if ext >= 4 else "cpu"
    steady = pct != 1.0
    cache = {}
    templates = []
    ext_reqs = [500, 100, 0, 1 << 39, 2000, 7, 1 << 20, 64][:n_classes] if n_classes <= 8 else [100 + 13 * k for k in range(n_classes)]
    if family == "mixed-tile":                                     # one 64-slot tile: tiny requests beside the two sentinels (rmin comes from another slot)
        ext_reqs = [1, 2, 3, I64_MAX, 5, I64_MIN + 1, 7, 8] + ext_reqs[8:]
    if family in ("prealloc-wrap", "filter-wrap"):
        ext_reqs = [500, 1 << 62, 100, (1 << 62) + (1 << 61), 0, -(1 << 62), 1 << 61, 64] + ext_reqs[8:]
    for k, e in enumerate(ext_reqs):
        rq = {"cpu": 250, "memory": [1 << 38, 1 << 39, 3 << 38][k % 3], key: e}   # 3 * 2^38: only the SECOND step covers it at pct 0.7
        if S:
            rq[SCALARS[1]] = 1
            if k % 4 == 3:
                del rq[key]                                        # sometimes the pod does not name the extreme key
        templates.append(rq)
    for gi in range(n_groups):
        nm = f"ns/g{gi}"
        mm = 10
        pg = nv.PodGroup(nm, mm)
        pgs = nv.PGS(pg)
        if steady:
            pgs.matched = 9 if gi == 1 else 1 + gi % 5             # group 1 leads: 900 per mille
        if steady or gi % 3:
            pgs.pod = nv.Pod(nm + "-rep", nm, dict(templates[gi % len(templates)]))
            mr = {"cpu": 0, "memory": (1 << 30) if steady else [1 << 30, 1 << 35, 3 << 35, 1 << 37][gi % 4], "pods": 0, "ephemeral-storage": 0}
            mr[key] = 0 if steady else [0, 50, 1 << 57, 0][gi % 4]  # first checks ask MinResources x 10: 1.25 * 2^40 of memory needs the second step
            if family in ("prealloc-wrap", "filter-wrap"):
                mr[key] = [1 << 61, (1 << 61) + (1 << 60), -(1 << 61), 1 << 62][gi % 4]   # MinResources x notFinished wraps (wrap_mul)
                if gi == 1:
                    pgs.matched = 5 if steady else 0               # notFinished = 5: 5 * 2^61 wraps
                    mr[key] = 1 << 61
            if S:
                mr[SCALARS[1]] = 0
            pg.min_resources = mr
        cache[nm] = pgs
    pods = []
    for i in range(n_pods):
        gi = (i * 5 + i // 12) % n_groups
        pods.append(nv.Pod(f"uid{i}", f"ns/g{gi}", dict(templates[(i * 7) % len(templates)])))
    return cache, pods


def build(family, pct=1.0, rows=CHUNK, n_groups=12, n_pods=96, n_classes=8):
    t = _table(family, pct, rows)
    S = 2 if family == "scalar-lane" else 0
    ext = 4 if S else soa.LANE_CPU
    names = SCALARS[:S]
    cache, pods = _groups_and_pods(family, t, pct, ext, S, n_groups, n_pods, n_classes)
    sc = dict(nodes=t.objects(), cache=cache, pods=pods, names=names, n_classes=1, denied=set(), permitted=set())
    nodes, fit, groups, spods, _ = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], names, 1)
    return Scene(family, pct, sc, nodes, fit, groups, spods, _single_queries(t, ext, S), ext, tuple(t.answers))


def joint_scene(order_by_group=True):
    """The sequential pass's first-fit prune keeps one number per node, min(free cpu << 20, free memory), and saturates the shift at
    +-2^42.  Nodes with free cpu above 2^42, below -2^42 and exactly 2^42 sit in later tiles behind nodes that hold nothing; the pods
    ask for cpu AND memory, so the joint bound decides which tiles are opened.  Without the saturation 2^44 << 20 is 0 and the tile
    that holds the right node is dropped."""
    n = 330
    nodes = []
    special = {70: (1 << 44, 0, 1 << 36), 135: (1 << 42, 0, 1 << 36), 140: (0, 1 << 43, 1 << 36), 200: ((1 << 42) + (1 << 41), 0, 1 << 34),
               263: (1 << 62, -(1 << 62), 1 << 36), 300: (1 << 62, 0, 1 << 40)}
    for i in range(n):
        cpu, used, mem = special.get(i, (100, 0, 1 << 20))
        a, r = nv.Resource(), nv.Resource()
        a.Add({"cpu": cpu, "memory": mem, "pods": 110})
        r.Add({"cpu": used, "memory": 0})
        nodes.append(nv.NodeInfo(a, r, 1))
    asks = [(1 << 43, 1 << 35), (1 << 42, 1 << 35), (1 << 43, 1 << 35), ((1 << 42) + 1, 1 << 33), (1000, 1 << 30), (1 << 42, 1 << 34),
            (1 << 61, 1 << 35), (1 << 43, 1 << 35), (1 << 42, 1 << 36), (500, 1 << 35), (1 << 44, 1 << 30), (1 << 42, 1 << 33)]
    cache = {}
    for gi in range(3):
        pg = nv.PodGroup(f"ns/j{gi}", 3)
        cache[pg.name] = nv.PGS(pg)
    pods = []
    for i, (c, m) in enumerate(asks * 2):
        grp = None if i % 4 == 3 else f"ns/j{i % 3}"
        pods.append(nv.Pod(f"uid{i}", grp, {"cpu": c, "memory": m}))
    if order_by_group:
        pods.sort(key=lambda p: p.group or "")
    sc = dict(nodes=nodes, cache=cache, pods=pods, names=[], n_classes=1, denied=set(), permitted=set())
    nd, fit, groups, spods, _ = nv.to_soa(nodes, cache, pods, [], 1)
    return Scene("joint-bound", 1.0, sc, nd, fit, groups, spods)


# ------------------------------------------------------------------------------------------------------------------------
# the classifier: plain Python ints and numpy over the oracle's node_left.  It reads no device code; it restates what ANY
# chunk-local scheme with a `max + offset` bound has to guard (256-row chunks, 64-row groups, 64-chunk windows).
# ------------------------------------------------------------------------------------------------------------------------
def _wrap(x):
    return nv.wrap64(int(x))


def classify(snap, cls, pct, req, present, first_k, fits):
    """-> dict of flags for the group that holds the oracle's first_k (None when the query is not covered anywhere).
    snap: orc.Snapshot.  Rows are the nodes the reference's loop does not skip (core.go:606-617), in list order."""
    left, lpres = snap.node_left(cls, pct)
    keep = (snap.nodes.flags & soa.NODE_SKIP_MASK) == 0
    rows_of = np.nonzero(keep)[0]
    left = left[:, keep]
    L, m = left.shape
    want = [int(req[j]) for j in range(4)] + [int(req[4 + s]) if (present >> s) & 1 else I64_MIN for s in range(L - 4)]
    if not fits:
        return None
    row = int(np.searchsorted(rows_of, first_k))
    assert rows_of[row] == first_k
    chunk, grp = row // CHUNK, row // GROUP
    flags = dict(row=row, group=grp, chunk=chunk, offset_out_of_range=False, group_risky=False, unguarded_bound_below_request=False,
                 group_far=grp >= 128, window=chunk // 64, offsets=[], maxima=[], bounds=[])
    for j in range(L):
        col = [int(x) for x in left[j]]
        off = 0
        for c in range(chunk):
            off = _wrap(off + sum(col[c * CHUNK:(c + 1) * CHUNK]))
        local, acc = [], 0
        for k in range(chunk * CHUNK, min(m, (grp + 1) * GROUP)):
            acc = _wrap(acc + col[k])
            if k >= grp * GROUP:
                local.append(acc)
        # the running sum the reference holds at first_k, rebuilt from the two parts: must satisfy the request (self-check)
        total = _wrap(off + local[row - grp * GROUP])
        scalar_absent = j >= 4 and not any((int(p) >> (j - 4)) & 1 for p in lpres[keep][: row + 1])
        assert total >= want[j] or (scalar_absent and want[j] in (0, I64_MIN)), (j, total, want[j])
        mx = max(local)
        bound = _wrap(mx + off)
        flags["offsets"].append(off)
        flags["maxima"].append(mx)
        flags["bounds"].append(bound)
        flags["offset_out_of_range"] |= not (-SAFE < off < SAFE)
        flags["group_risky"] |= any(x >= SAFE or x <= -SAFE for x in local)
        flags["unguarded_bound_below_request"] |= bound < want[j]
    return flags


def classify_queries(orc, scene, queries=None):
    """[(query, oracle's (fits, first_k), flags)] for the scene's single queries"""
    snap = orc.Snapshot(scene.nodes, scene.fit)
    out = []
    for q in (scene.queries if queries is None else queries):
        cls, pct, req, pres = q
        ok, fk, _ = snap.compare_cluster(cls, req, pres, pct)
        out.append((q, (ok, fk), classify(snap, cls, pct, req, pres, fk, ok)))
    return out


def batch_queries(orc, scene, exp):
    """the node scans a batch asks for, rebuilt on the host: one per pod with a reservation verdict (core.go:157-161) or a first-check
    verdict of a gang that came with its MinResources: (pod, query)"""
    g, p, S = scene.groups, scene.pods, scene.S
    out = []
    for i in range(p.p):
        code, own = int(exp.pf_code[i]), int(p.group[i])
        if code in (soa.PF_PASS_FIRST_FITS, soa.PF_REJECT_FIRST) and g.flags[own] & soa.GROUP_HAS_MINRES and g.flags[own] & soa.GROUP_HAS_POD:
            pre, ppres = orc.pre_allocated(g, own, 0, S)            # first check (core.go:136-147): the gang's own MinResources x notFinished, pct 1.0
            out.append((i, (int(g.cls[own]), 1.0, pre, ppres)))     # (gangs captured inside the batch are left out: their default is the pod's request)
        if code not in (soa.PF_PASS_RESERVE_FITS, soa.PF_REJECT_RESERVE):
            continue
        ld = int(exp.pf_leader[i])
        pre, ppres = orc.pre_allocated(g, ld, int(g.matched[ld]), S)
        req = [nv.wrap64(pre[j] + int(p.req[j, i])) for j in range(4)]
        pres = ppres | int(p.req_present[i])
        for s in range(S):
            has = (int(p.req_present[i]) >> s) & 1
            req.append(nv.wrap64(pre[4 + s] + (int(p.req[4 + s, i]) if has else 0)))
        out.append((i, (int(g.cls[ld]), 0.7, req, pres)))
    return out
