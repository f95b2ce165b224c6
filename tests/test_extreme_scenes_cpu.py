"""CPU side of the int64-extremes tests: (1) every scene family of tests/extreme_scenes.py is what it claims — the classifier, plain
Python ints over the oracle's node_left, finds queries whose answer an UNGUARDED `max + offset` bound would prune away; (2) on small
versions of every family the two independent oracle statements (oracle/bs_oracle.c and oracle/naive_ref.py, Python ints + wrap64)
agree on compare_cluster, scan_prefix and a whole batch, and the C sequential pass agrees with the object-level replay.  The scenes are
meant for a GPU comparison with the C oracle, chain by chain; that comparison is not part of the suite yet."""
import numpy as np
import pytest

import extreme_scenes as xs
import naive_ref as nv
import seq_obj_replay as sor
from test_oracle_vs_naive import _check_scene
from test_seq_oracle_pin import _assert_same, _c_pass

TUNINGS = (1.0, 0.7)
SMALL = 64                      # rows per "chunk" of the small layouts: N <= 400 everywhere
SEQ_FAMILIES = ("offset-high", "risky-group", "wrap-and-return")


def _flagged(res, **want):
    return [r for r in res if r[2] is not None and all(r[2][k] == v for k, v in want.items())]


@pytest.mark.parametrize("pct", TUNINGS)
@pytest.mark.parametrize("family", xs.SINGLE_FAMILIES)
def test_family_is_what_it_claims(family, pct, orc):
    scene = xs.build(family, pct, n_groups=3, n_pods=6)
    res = xs.classify_queries(orc, scene)
    covered = _flagged(res)
    assert len(covered) >= 8 and len(covered) < len(res), "the battery has covered and uncovered queries"
    assert {fk for _, (ok, fk), _ in res if ok} & set(scene.answers), "no query is decided by the ordinary lane"
    need = _flagged(res, unguarded_bound_below_request=True)
    if family in xs.MUST_NEED_A_GUARD or family.startswith(("risky", "wrap")):
        assert need, "no query of this family needs a guard: an unguarded scan would give the right answers"
        assert any(q[1] == pct for q, _, _ in need), "... at the percentage the scene is tuned for"
    if family in ("offset-high", "offset-low", "far", "far-window", "scalar-lane"):
        only = _flagged(res, unguarded_bound_below_request=True, offset_out_of_range=True, group_risky=False)
        assert only, "the offset guard alone has to save some query (the group's local sums are small)"
        sign = -1 if family == "offset-low" else 1
        assert all(sign * r[2]["offsets"][scene.ext] >= xs.SAFE for r in only)
    if family.startswith("risky-group"):
        assert _flagged(res, unguarded_bound_below_request=True, offset_out_of_range=False, group_risky=True), "the table's `risky` mark alone"
    if family.startswith("wrap-and-return"):
        snap = orc.Snapshot(scene.nodes, scene.fit)
        pre = {p: snap.scan_prefix(0, p)[0][scene.ext] for p in TUNINGS}
        s = np.sign(pre[pct])
        s = s[s != 0]
        assert int(np.sum(s[1:] != s[:-1])) >= 2, "the reference sum changes sign by wrapping and comes back"

        def changes(r):
            t = np.sign(pre[r[0][1]][: r[2]["row"] + 1])
            t = t[t != 0]
            return int(np.sum(t[1:] != t[:-1]))
        assert any(changes(r) >= 2 for r in need), "a first covering row lies behind the wrap AND the return"
    if family == "totals-edge":
        snap = orc.Snapshot(scene.nodes, scene.fit)
        left, _ = snap.node_left(0, pct)
        tot = [nv.wrap64(sum(int(x) for x in left[scene.ext, c * xs.CHUNK:(c + 1) * xs.CHUNK])) for c in range(5)]
        assert tot[:4] == [0, -1, xs.I64_MIN, 1 << 40] and tot[3] & 0xFFFFFFFF == 0, tot
        assert {r[2]["chunk"] for r in covered} >= {4}
    if family in ("far", "far-window"):
        assert _flagged(res, unguarded_bound_below_request=True, group_far=True)
    if family == "far-window":
        assert any(r[2]["window"] >= 1 for r in need), "the answer's chunk lies in the second 64-chunk window"
        assert scene.nodes.n > 16384
    if family == "scalar-lane":
        assert scene.S == 2 and scene.ext == 4
        first_key = int(np.nonzero(scene.nodes.allocatable_present & 1)[0][0])
        assert 0 < first_key < xs.CHUNK and first_key % 64, "the key first appears inside a chunk, off a group boundary"
        assert any(q[3] == 0b10 for q, (ok, _), _ in res if ok), "a covered query that does not name the extreme key"


@pytest.mark.parametrize("pct", TUNINGS)
@pytest.mark.parametrize("family", xs.BATCH_FAMILIES)
def test_batch_scene_asks_scans_that_need_a_guard(family, pct, orc, soa):
    """the scans a batch asks for — reservation checks in the steady state (pct 0.7), first checks where nobody has matched pods
    (pct 1.0) — rebuilt on the host, are the oracle's, and some of them need a guard"""
    scene = xs.build(family, pct)
    assert scene.nodes.n <= 1400 and scene.pods.p <= 600 and scene.groups.g <= 40
    snap = orc.Snapshot(scene.nodes, scene.fit)
    exp = orc.Sop(snap, scene.groups).batch(scene.pods, soa.STAGE_ALL)
    bq = xs.batch_queries(orc, scene, exp)
    assert len(bq) >= 5
    need = 0
    for i, (cls, pct, req, pres) in bq:
        ok, fk, _ = snap.compare_cluster(cls, req, pres, pct)
        assert fk == int(exp.pf_first_k[i]) and ok == (int(exp.pf_code[i]) in (soa.PF_PASS_RESERVE_FITS, soa.PF_PASS_FIRST_FITS))
        f = xs.classify(snap, cls, pct, req, pres, fk, ok)
        need += bool(f and f["unguarded_bound_below_request"])
    assert need, "no scan of this batch needs a guard"
    if family == "mixed-tile":
        asked = {int(x) for x in scene.pods.req[scene.ext]}
        assert {xs.I64_MAX, xs.I64_MIN + 1, 1, 2} <= asked
    if family == "prealloc-wrap" and pct == 0.7:
        ld = int(exp.pf_leader[bq[0][0]])
        g = scene.groups
        nf = int(g.min_member[ld]) - int(g.matched[ld])
        mr = int(g.min_resources[scene.ext, ld])
        assert nf >= 4 and mr * nf >= 1 << 63 and orc.pre_allocated(g, ld, int(g.matched[ld]), 0)[0][scene.ext] == nv.wrap64(mr * nf)
        assert any(int(scene.pods.req[scene.ext, i]) + nv.wrap64(mr * nf) < xs.I64_MIN for i, _ in bq), "pod + preallocated wraps too"
    if family == "filter-wrap":
        free = [int(a) - int(r) for a, r in zip(scene.nodes.allocatable[0], scene.nodes.requested[0])]
        assert any(x > xs.I64_MAX for x in free) and any(x < xs.I64_MIN for x in free), "allocatable - requested wraps both ways"


def _resource(req, present, names):
    r = nv.Resource(MilliCPU=req[0], Memory=req[1], EphemeralStorage=req[2], AllowedPodNumber=req[3])
    for s, nm in enumerate(names):
        if (present >> s) & 1:
            r.ScalarResources = r.ScalarResources or {}
            r.ScalarResources[nm] = req[4 + s]
    return r


def _small(family, pct, **kw):
    return xs.build(family, pct, rows=SMALL, **kw)


@pytest.mark.parametrize("pct", TUNINGS)
@pytest.mark.parametrize("family", xs.SINGLE_FAMILIES)
def test_small_single_queries_both_oracles_agree(family, pct, orc, soa):
    scene = _small(family, pct, n_groups=3, n_pods=6)
    assert scene.nodes.n <= 400
    snap = orc.Snapshot(scene.nodes, scene.fit)
    names, rep = scene.sc["names"], nv.Pod("rep", None, {}, cls=0)
    for p in TUNINGS:
        pre, pres, idx = snap.scan_prefix(0, p)
        total = nv.Resource()
        for k, info in enumerate(scene.sc["nodes"]):
            total.Add(nv.single_node_resource(info, rep, p).ResourceList())
            lanes, mask = nv._lanes(total, names)
            assert pre[:, k].tolist() == lanes and int(pres[k]) == mask and int(idx[k]) == k, (family, p, k)
    seen = set()
    for cls, p, req, present in scene.queries:
        ok, fk, _ = snap.compare_cluster(cls, req, present, p)
        ok_n, fk_n = nv.compare_cluster(scene.sc["nodes"], rep, _resource(req, present, names), p)
        assert (ok, fk if ok else None) == (ok_n, fk_n), (family, p, req, present)
        seen.add(fk)
    assert len(seen) >= 3


@pytest.mark.parametrize("pct", TUNINGS)
@pytest.mark.parametrize("family", xs.BATCH_FAMILIES)
def test_small_batches_both_oracles_agree(family, pct, orc, soa):
    scene = _small(family, pct, n_pods=48)
    out = _check_scene(scene.sc, orc, soa, (family, pct))
    assert (out.pf_first_k != soa.K_NOT_SCANNED).sum() >= 5, "the batch asks for node scans"


@pytest.mark.parametrize("run_filter", [False, True], ids=["prefilter", "prefilter+filter"])
@pytest.mark.parametrize("pct", TUNINGS)
@pytest.mark.parametrize("family", SEQ_FAMILIES + ("joint-bound",))
def test_small_sequential_pass_both_statements_agree(family, pct, run_filter, orc, soa):
    if family == "joint-bound":
        scene = xs.joint_scene()
    else:
        scene = _small(family, pct, n_pods=48, n_classes=2)
        scene.sc["pods"].sort(key=lambda p: p.group)
    stages = soa.STAGE_PREFILTER | (soa.STAGE_FILTER if run_filter else 0)
    c, _ = _c_pass(orc, soa, scene.sc, (), stages)
    obj = sor.replay(scene.sc, (), run_filter=run_filter, scalar_names=scene.sc["names"])
    _assert_same(soa, obj, c, (family, pct))
    if family == "joint-bound":
        assert {70, 135, 300} <= set(c["pod_node"].tolist()), "the nodes behind the saturated bound take pods"
