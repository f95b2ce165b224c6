"""GPU: the whole-step launch's gang-aligned pod ranges (bs_pod_ranges.hpp) and the Permit quorum closed in LDS for gangs inside one range
(tally_tail_whole, bs_fast.hpp), against the CPU oracle, every output array.  The queues are built so that the layout has to deal with its edge
cases: gangs across every 256-pod boundary, a gang of more than 256 pods, a queue without any cut, ungrouped pods and gangs with no pod."""
import numpy as np
import pytest

from test_gpu_parity import assert_batch_equal, load_ctx

pytestmark = pytest.mark.gpu


def _scene(bsa, soa, config, kind, seed=7):
    nodes, fit, groups, pods, _ = bsa.synth.make(config, "tail", seed=seed)
    pods = pods.copy()
    P, G = pods.p, groups.g
    grp = np.array(pods.group, copy=True)
    if kind == "straddle":                      # a gang of four pods across every 256-pod boundary
        for k in range(1, (P + 255) // 256):
            grp[max(0, 256 * k - 2):min(P, 256 * k + 2)] = k % G
    elif kind == "big":                         # one gang of 300 pods
        grp[100:400] = 0
        grp[(grp == 0) & ((np.arange(P) < 100) | (np.arange(P) >= 400))] = 1 % G
    elif kind == "interleaved":                 # every gang spans the queue: no cut at all
        grp[:] = np.arange(P) % min(G, 7)
    elif kind == "ungrouped":                   # ungrouped pods everywhere, and the upper half of the groups without a pod
        grp[:] = np.minimum(grp, G // 2 - 1)
        grp[np.random.default_rng(seed).random(P) < 0.2] = soa.POD_NOT_GROUPED
    pods.group[:] = grp
    return nodes, fit, groups, pods


KINDS = ["synth", "straddle", "big", "interleaved", "ungrouped"]


@pytest.mark.parametrize("config", ["cfg2", "cfg3"])
@pytest.mark.parametrize("kind", KINDS)
def test_gang_ranges_equal_the_oracle(config, kind, bsa, soa, orc):
    nodes, fit, groups, pods = _scene(bsa, soa, config, kind)
    exp = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        for n in range(4):                     # the first batches over a fresh queue may take another form; the later ones the whole step
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp, f"{config}/{kind} batch {n}")
        for stages in (soa.STAGE_PREFILTER | soa.STAGE_TALLY, soa.STAGE_PREFILTER):
            e = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, stages)
            g = ctx.batch(stages)
            for name in ("pf_code", "pf_first_k", "pf_leader", "fl_code", "fl_feasible"):
                assert np.array_equal(getattr(g, name), getattr(e, name)), (kind, stages, name)
            if stages & soa.STAGE_TALLY:
                assert np.array_equal(g.group_admit, e.group_admit) and np.array_equal(g.group_ready, e.group_ready), (kind, stages)


@pytest.mark.parametrize("kind", ["synth", "straddle", "ungrouped"])
def test_gang_ranges_with_filter_deny_and_host_results(kind, bsa, soa, orc):
    nodes, fit, groups, pods = _scene(bsa, soa, "cfg2", kind)
    fd = soa.STAGE_ALL | soa.BATCH_FILTER_DENY
    exp_fd = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, fd, bitmap=False)
    exp = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        for n in range(3):
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp, f"{kind} batch {n}")
            assert_batch_equal(ctx.batch(fd, bitmap=False, rows=False), exp_fd, f"{kind} Filter-deny batch {n}", bitmap=False)
            ctx.run(soa.STAGE_ALL | soa.BATCH_HOST_RESULTS)
            out = ctx.read(bitmap=False)
            assert_batch_equal(out, exp, f"{kind} host-results batch {n}", bitmap=False)


def test_gang_ranges_with_commit(bsa, soa, orc):
    nodes, fit, groups, pods = _scene(bsa, soa, "cfg2", "straddle")
    stages = soa.STAGE_ALL | soa.BATCH_COMMIT
    sop = orc.Sop(orc.Snapshot(nodes, fit), groups)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        for n in range(3):
            assert_batch_equal(ctx.batch(stages, bitmap=False), sop.batch(pods, stages, bitmap=False), f"commit batch {n}", bitmap=False)


@pytest.mark.parametrize("config", ["cfg2", "cfg3"])
def test_gang_ranges_after_apply_then_a_fresh_load(config, bsa, soa, orc):
    """bs_pods_apply moves positions on the device: 256 pods per block until the next bs_pods_load, which lays the ranges out again"""
    nodes, fit, groups, pods = _scene(bsa, soa, config, "straddle")
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        for _ in range(2):
            ctx.batch(soa.STAGE_ALL)
        rm = np.arange(5, 60, 3, dtype=np.uint32)
        ins = pods.take(np.arange(300, 340))
        pods2 = pods.patched(remove=rm, insert=ins, insert_at=None)
        ctx.apply_pods(remove=rm, insert=ins)
        exp2 = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods2, soa.STAGE_ALL)
        for n in range(3):
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp2, f"{config} after apply, batch {n}")
        ctx.load_pods(pods2)
        for n in range(3):
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp2, f"{config} after a fresh load, batch {n}")


def test_gang_ranges_sharded_world_two_on_one_gpu(bsa, soa, orc):
    """the sharded run (two ranks of one job on one GPU, gloo collective) keeps the returning-atomic-free path off (no quorum on a rank)"""
    from test_gpu_multirank import _check, _run
    from multirank_worker import with_early_returners
    config, scenario, seed = "cfg2", "tail", 5
    nodes, fit, groups, pods, _ = bsa.synth.make(config, scenario, seed=seed)
    pods = with_early_returners(pods, soa, seed)
    exp = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)
    res = _run("gloo-partitioned", 2, config, scenario, seed)
    assert all(str(d["status"]) == "ok" for d in res), [str(d["status"]) for d in res]
    _check(res, "gloo-partitioned", bsa, soa, orc, config, scenario, seed, pods, groups, exp)
