"""Every scalar-lane count 0..BS_MAX_SCALARS through every family of lane-templated kernels the host dispatches (csrc/bs_lanes.hpp):
the batch chains (general / positional, steady in its one-launch and two-launch forms, the general chain forced, early Filter), the
sequential pass and the Permit timeout, the victim search, the preemption plans with APPLY, and the bound table's patch and remap.
Shapes are the smallest at which these launches still do all their work: about 70 nodes (more than one 64-node word), 70 pods, 4 groups.
The comparisons are the suite's own, bit for bit: the oracle for the batches, the CPU restatements in tests/ for the rest.  The throughput
regime's launches need thousands of distinct request classes and stay with tests/test_gpu_throughput.py."""
import functools

import numpy as np
import pytest

import naive_ref as nv
import preempt_gang_scenes as gs
import preempt_ref as pr
import scenarios
import test_gpu_bound_apply_nodes as t_apply_nodes
import test_gpu_bound_nodes as t_bound_nodes
import test_gpu_preempt as t_preempt
import test_gpu_preempt_commit as t_commit
import test_gpu_preempt_gang as t_gang
from preempt_scenes import random_scene
from test_gpu_parity import _batch_case, _force_class_mode, assert_batch_equal, load_ctx
from test_gpu_seq_expire import Case, waiting_scene

pytestmark = pytest.mark.gpu
LANES = range(13)                                       # 0..BS_MAX_SCALARS (include/bsched.h)
NAMES = [f"example.com/r{i}" for i in range(12)]        # the scene builder's own list stops at two scalar resources
N_NODES, N_PODS, N_GROUPS, N_CLASSES = 70, 70, 4, 3
# the environment switches of the existing chain tests (test_gpu_fastpath.py, test_gpu_epoch.py, test_gpu_parity.py)
CHAINS = {
    "default": {},
    "general": {"BS_NO_FAST": "1", "BS_NO_EPOCH": "1"},
    "general+early-filter": {"BS_NO_FAST": "1", "BS_NO_EPOCH": "1", "BS_EARLY_FILTER_MIN": "0"},
    "two-launch": {"BS_STEP_A": "0"},
    "one-launch+final": {"BS_STEP_A": "2"},             # k_fast_step_a<S, false> + k_fast_final; the default is the whole step in one launch
}


def test_the_lane_range_is_the_headers():
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bsched.h")).read()
    assert int(re.search(r"BS_MAX_SCALARS = (\d+)", h).group(1)) == LANES[-1] == len(NAMES)


@functools.lru_cache(maxsize=None)
def _scene(S):
    """the random scene builder with n_scalars = S, over a list of twelve scalar names"""
    saved = scenarios.SCALARS
    scenarios.SCALARS = NAMES
    try:
        sc = scenarios.random_objects(9100 + S, n_nodes=N_NODES, n_groups=N_GROUPS, n_pods=N_PODS, n_scalars=S, n_classes=N_CLASSES)
    finally:
        scenarios.SCALARS = saved
    assert len(sc["names"]) == S
    return sc


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("S", LANES)
def test_batches(S, chain, monkeypatch, bsa, soa, orc):
    for k, v in CHAINS[chain].items():
        monkeypatch.setenv(k, v)
    sc = _scene(S)
    # the scene as generated: a what-if batch and a committing one over one queue (the general or the positional chain)
    _batch_case(sc, bsa, soa, orc)
    # the same scene forced into the steady state (every group has its pod and MinResources, the leader has matched pods): the first batch
    # over a fresh queue takes the chain's two-launch form at most, the later ones the one-launch form where it applies
    nodes, fit, groups, pods, _ = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], denied=sc["denied"], permitted=sc["permitted"])
    assert nodes.lanes == 4 + S
    rng = np.random.default_rng(S)
    _force_class_mode(groups, rng, N_CLASSES)
    groups.matched[:] = rng.integers(1, 4, groups.g)
    exp = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        for i in range(3):
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp, f"S={S} {chain}: steady scene, batch {i}")
        st = ctx.stats(soa.STAGE_ALL)                   # (an instrumented batch: it never takes a one-launch form, so it tells the chain only)
        print(f"S={S} {chain}: fast_path {st['fast_path']} launches {st['launches']} class_mode {st['class_mode']}")
        assert st["fast_path"] == (0 if "BS_NO_FAST" in CHAINS[chain] else 1), st
        assert_batch_equal(ctx.batch(soa.STAGE_ALL | soa.BATCH_COMMIT), exp, f"S={S} {chain}: steady scene, committing batch")


@pytest.mark.parametrize("S", LANES)
def test_sequential_pass_then_every_waiting_gang_expires(S, bsa, soa, orc):
    """the first 60 nodes are unschedulable: the 70 waiting pods of four gangs sit on nodes 60..64, fourteen a node, across the boundary of
    the first 64-node word; every second node lacks the scalar keys, which the assume step then creates"""
    with Case(bsa, soa, orc, waiting_scene(soa, [20, 17, 18, 15], n_nodes=N_NODES, S=S, pods_cap=14, skip_nodes=60, interleave=True, seed=300 + S)) as c:
        assert int((c.st.wait_node >= 0).sum()) == N_PODS and int(c.st.wait_node.max()) >= 64
        e = c.expire(f"S={S}", all=True, deny=True)
        assert e["n_groups"] == 4 and e["n_pods"] == N_PODS and not np.any(c.st.wait_node >= 0)
        c.follow_up(f"S={S}")


@pytest.mark.parametrize("S", LANES)
def test_victim_search(S):
    sc = random_scene(7300 + S, n=N_NODES, per_node=(2, 9), S=S, q=65, groups=N_GROUPS, p=N_PODS, fit_density=0.6)
    exp = pr.preempt_np(pr.Prep(sc["nodes"], sc["bound"], sc["S"]), sc["fit"], sc["pods"], sc["pod_index"], sc["priority"], sc["protected"], 6)
    assert np.any(exp["node"] >= 0) and np.any(exp["n_victims"] > 0), "the scene places nobody: nothing to pick"
    t_preempt._run_and_check(sc, cap=6, where=f"S={S}")


@pytest.mark.parametrize("S", LANES)
def test_preemption_plan_with_apply(S):
    sc = t_commit.commit_scene(8300 + S, n=N_NODES, per_node=(2, 9), S=S, q=65, groups=N_GROUPS, p=N_PODS, fit_density=0.6)
    exp = t_commit._expect(sc, 6, True, True)
    assert np.any(exp["res"]["n_victims"] > 0), "the scene evicts nobody: APPLY has nothing to write"
    with t_commit._ctx(sc) as ctx:
        got = ctx.preempt_commit(sc["pod_index"], sc["priority"], sc["protected"], victim_cap=6, apply=True, assume=True)
        t_commit._compare(got, exp["res"], f"S={S}")
        t_commit._compare_state(ctx, exp, f"S={S}")


@pytest.mark.parametrize("S", LANES)
def test_gang_plan_with_apply(S):
    sc = gs.gang_scene(8500 + S, n=N_NODES, per_node=(2, 9), S=S, q=65, groups=N_GROUPS)
    t_gang._check(sc, 6, modes=((True, True),), where=f"S={S}")


@pytest.mark.parametrize("S", LANES)
def test_bound_table_patch_with_node_requests(S):
    t_apply_nodes.test_node_requests_and_table_equal_the_model_after_every_step(S, N_NODES)


@pytest.mark.parametrize("S", LANES)
def test_bound_table_follows_node_list_surgery(S):
    t_bound_nodes.test_table_equals_the_model(S, N_NODES)
