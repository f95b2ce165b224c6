"""GPU parity of the throughput regime's NODE WORDS (node_words_block in csrc/bs_fast.hpp, read by the lean Filter items of csrc/bs_filter_t.hpp) at the
node counts and table selections where their layout can go wrong, bit for bit against the oracle.

Launch A writes three tables of (ok, ~holds) word pairs, one pair per 64 nodes, from cdiv(N, 256) blocks of four waves.  With N mod 256 in [1, 64] the
last block's fourth wave has no node and its word index is the table's stride: before the guard of csrc/bs_nodew_layout.hpp it stored (ok = 0) onto
pair 0 of the NEXT table, racing with block 0's valid store, and Filter then failed nodes 0..63 for every slot that read that table.  Table 0 is never
hit; table 1 is read for a STALE leader (sop.maxFinishedPG carried into the batch), table 2 for a leader whose MinResources names a non-zero scalar.

A race does not lose every time: these scenes are a NET, four batches per context.  The DETECTOR of the defect is tests/test_nodew_layout_cpu.py, which
walks every store of the grid on the CPU through the same header the kernels call.

Node counts by residue N mod 256: 1, 20, 63, 64 (the last wave overhangs) and 65, 128, 255, 0 (controls), around 300 and around 1300.  Every scene
asserts its own preconditions on the oracle's result before it touches the GPU, so that it cannot go vacuous: the regime (at least 1024 distinct
evaluated requests), the table (one leader among the evaluated pods, two for the stale-leader kind, a non-zero scalar MinResources for kind 2), and at
least 100 evaluated pods whose bitmap has a bit in word 0 — otherwise ok = 0 on nodes 0..63 would change nothing.

Every test needs a real MI355X (`-m gpu`); nothing falls back to the CPU."""
import functools
import importlib

import numpy as np
import pytest

import orc
from test_gpu_parity import assert_batch_equal, load_ctx
from test_gpu_throughput import _check_split

pytestmark = pytest.mark.gpu

bsa_mod = importlib.import_module("batch-scheduler_amd")
soa = bsa_mod.soa

RESIDUES = (1, 20, 63, 64, 65, 128, 255, 0)
NODE_COUNTS = [256 + r for r in RESIDUES] + [1280 + r if r else 1536 for r in RESIDUES]
FORMS = ["default", "5", "7", "8"]           # every form of the Filter role that reads node words (BS_TP_FILTER >= 5; the default is 6)
SWITCHES = ("BS_TP_FILTER", "BS_TP_SHARE", "BS_TP_FWAVES", "BS_FILTER_WAVES", "BS_TP_SPLIT", "BS_TP_TMIN", "BS_NO_NODEW")
BATCHES = 4


def _set_form(monkeypatch, form, tmin=None):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if form != "default":
        monkeypatch.setenv("BS_TP_FILTER", form)
    if tmin is not None:
        monkeypatch.setenv("BS_TP_TMIN", str(tmin))
    return 6 if form == "default" else int(form)


def _preconditions(what, pods, groups, exp, n_leaders, scalar_leader=False):
    ev = exp.fl_code == soa.FL_EVALUATED
    reqs = np.unique(np.concatenate([pods.req[:, ev], pods.req_present[None, ev].astype(np.int64), pods.cls[None, ev].astype(np.int64)]), axis=1).shape[1]
    assert reqs >= 1024, f"{what}: {reqs} distinct evaluated requests: not the throughput regime"
    leaders = np.unique(exp.pf_leader[ev])
    assert len(leaders) == n_leaders and leaders.min() >= 0, f"{what}: leaders among the evaluated pods: {leaders.tolist()}"
    S = groups.min_resources.shape[0] - 4
    scalar = [bool(np.any((groups.min_resources[4:, l] != 0) & (((groups.min_resources_present[l] >> np.arange(S)) & 1) != 0))) for l in leaders]
    if scalar_leader:
        assert all(scalar), f"{what}: the leader's MinResources carries no scalar: table 2 is not selected"
    else:
        assert not any(scalar), f"{what}: a leader's MinResources carries a scalar: table 2 would be selected"
    word0 = int(np.count_nonzero(exp.fl_bitmap[0, ev]))
    assert word0 >= 100, f"{what}: only {word0} evaluated pods pass a node among 0..63"


@functools.lru_cache(maxsize=None)
def _synthetic(n_nodes, lane):
    """kind 0 (lane None): all-distinct requests, one leader without a scalar MinResources -> table 0.  kind 2: the same scene, the leader the oracle
    names gets MinResources[lane] = 1 -> no node can hold a member (getLeftResource has no scalars) -> table 2."""
    nodes, fit, groups, pods, _ = bsa_mod.synth.make("cfg3", "busy", pods=2000, groups=400, nodes=n_nodes, classes=8, scalars=2)
    pods.req[0, :] += np.arange(pods.p, dtype=np.int64)
    exp = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)
    what = f"N = {n_nodes}, table 0"
    if lane is not None:
        ev = exp.fl_code == soa.FL_EVALUATED
        leaders = np.unique(exp.pf_leader[ev])
        assert len(leaders) == 1
        groups.min_resources[lane, leaders[0]] = 1
        groups.min_resources_present[leaders[0]] |= np.uint32(1 << (lane - 4))
        exp = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)
        what = f"N = {n_nodes}, table 2 (scalar lane {lane})"
    _preconditions(what, pods, groups, exp, 1, scalar_leader=lane is not None)
    return nodes, fit, groups, pods, exp


def _run_synthetic(n_nodes, lane, form, monkeypatch, tmin=None):
    nodes, fit, groups, pods, exp = _synthetic(n_nodes, lane)
    f = _set_form(monkeypatch, form, tmin)
    with load_ctx(bsa_mod, nodes, fit, groups, pods) as ctx:
        for k in range(BATCHES):
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp, f"N = {n_nodes}, table {0 if lane is None else 2}, form {form}, batch {k}")
        _check_split(ctx.stats(soa.STAGE_ALL), f)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_nodes", NODE_COUNTS)
def test_table_0_one_leader(n_nodes, form, monkeypatch):
    _run_synthetic(n_nodes, None, form, monkeypatch)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_nodes", NODE_COUNTS)
def test_table_2_leader_with_a_scalar_min_resources(n_nodes, form, monkeypatch):
    _run_synthetic(n_nodes, 5, form, monkeypatch)


@pytest.mark.parametrize("form", FORMS)
def test_table_2_first_scalar_lane_at_1300_nodes(form, monkeypatch):
    """The scene the defect was described on: N = 1300 (N mod 256 = 20), the leader's MinResources names one unit of the FIRST scalar resource."""
    _run_synthetic(1300, 4, form, monkeypatch)


@pytest.mark.parametrize("n_nodes,lane", [(276, None), (276, 5), (1300, None), (1300, 5), (1344, 5)])
def test_two_tiles_per_wave_read_the_tables_too(n_nodes, lane, monkeypatch):
    """BS_TP_TMIN=1: the transposed items take PAIRS of tiles (filter_item_multi) from the first tile on."""
    _run_synthetic(n_nodes, lane, "default", monkeypatch, tmin=1)


@functools.lru_cache(maxsize=None)
def _stale(n_nodes):
    """kind 1, in the manner of test_random_scenes_with_stale_leader_every_form (test_gpu_throughput.py; its random object scenes evaluate fewer than 1024
    pods, so this one stands on the synthetic cluster): batch A commits and leaves a leader behind, the group state is changed so that batch B computes
    another one, and the head of the queue carries a lastPermittedPod entry (core.go:95-98): those pods pass PreFilter without reaching findMaxPG and
    evaluate Filter against the STALE leader -> table 1.  The oracle plays batch A here; the GPU's state after ITS batch A is held against the oracle's
    before anything is edited."""
    nodes, fit, groups, pods, _ = _synthetic(n_nodes, None)
    sop = orc.Sop(orc.Snapshot(nodes, fit), groups)
    exp_a = sop.batch(pods, soa.STAGE_ALL)
    after_a = sop.groups.copy()
    stale = sop.leader
    assert stale >= 0 and not after_a.state_equal(groups)
    groups_b = after_a.copy()
    _edit_for_batch_b(groups_b, stale)
    sop.groups.flags[:], sop.groups.matched[:], sop.groups.min_member[:] = groups_b.flags, groups_b.matched, groups_b.min_member
    pods_b = pods.take(np.arange(pods.p))
    pods_b.flags[:150] |= soa.POD_LAST_PERMITTED
    exp_b = sop.batch(pods_b, soa.STAGE_ALL)
    what = f"N = {n_nodes}, table 1"
    _preconditions(what, pods_b, groups_b, exp_b, 2)
    ev = exp_b.fl_code == soa.FL_EVALUATED
    on_stale = ev & (exp_b.pf_leader == stale) & ((pods_b.flags & soa.POD_LAST_PERMITTED) != 0)
    assert int(np.count_nonzero(exp_b.fl_bitmap[0, on_stale])) >= 100, f"{what}: too few pods evaluated against the stale leader pass a node among 0..63"
    return nodes, fit, groups, pods, exp_a, after_a, stale, pods_b, exp_b


def _edit_for_batch_b(g, stale):
    """the deny entries expire, the old leader falls back and a neighbour becomes the gang closest to completion"""
    g.flags &= ~np.uint8(soa.GROUP_DENIED)
    new = (stale + 5) % g.g
    g.matched[stale] = 0
    g.min_member[new] = 64
    g.matched[new] = 30


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_nodes", NODE_COUNTS)
def test_table_1_stale_leader(n_nodes, form, monkeypatch):
    nodes, fit, groups, pods, exp_a, after_a, stale, pods_b, exp_b = _stale(n_nodes)
    f = _set_form(monkeypatch, form)
    with load_ctx(bsa_mod, nodes, fit, groups, pods) as ctx:
        assert_batch_equal(ctx.batch(soa.STAGE_ALL | soa.BATCH_COMMIT), exp_a, f"N = {n_nodes}, batch A")
        g2 = ctx.read_groups()
        assert g2.state_equal(after_a)
        _edit_for_batch_b(g2, stale)
        ctx.load_groups(g2)
        ctx.load_pods(pods_b)
        for k in range(BATCHES):
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp_b, f"N = {n_nodes}, table 1, form {form}, batch B {k}")
        _check_split(ctx.stats(soa.STAGE_ALL), f)
