"""The context's pinned staging buffers where they can go wrong: the call that makes one GROW while the copy or kernel of the call
before may still be reading it (csrc/bs_hostmem.hpp, PinnedBuf::reserve), and the context's lifetime (every stream, event and
buffer released by bs_destroy).  The shapes are the smallest that cross each buffer's first capacity; results are compared with
what the suite already trusts — read-back for loads, the oracle for batches."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import assert_batch_equal, load_ctx

pytestmark = pytest.mark.gpu

GROUP_FIELDS = ("min_member", "status_scheduled", "matched", "flags", "cls", "min_resources", "min_resources_present", "occupied_by")


@pytest.fixture(scope="module")
def big(bsa):
    """150 nodes, 2 048 groups, 4 096 pods (5 lanes): the large second load of the pod and group cases"""
    nodes, fit, groups, pods, _ = bsa.synth.make("tiny", "tail", pods=4096, groups=2048)
    return nodes, fit, groups, pods


@pytest.fixture(scope="module")
def tiny(bsa, soa, orc):
    """the 96-pod scene, its first 8 pods, and the oracle's batch over those 8"""
    nodes, fit, groups, pods, _ = bsa.synth.make("tiny", "tail")
    pods8 = pods.take(np.arange(8))
    exp8 = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods8, soa.STAGE_ALL)
    return nodes, fit, groups, pods, pods8, exp8


def test_pod_staging_grows_behind_a_load_in_flight(big, bsa):
    """h_stage: 8 pods, then at once 4 096 — the second load waits for the first upload, frees the buffer it read and packs into a
    larger one; the resident queue is the second input."""
    nodes, fit, groups, pods = big
    with load_ctx(bsa, nodes, fit, groups, pods.take(np.arange(8))) as ctx:
        ctx.load_pods(pods)
        assert ctx.read_pods().equal(pods)


def test_group_staging_grows_behind_a_load_in_flight(big, bsa, soa):
    """h_gstage: 4 groups, one delta, then 2 048 groups; the read-back is the second load."""
    nodes, fit, groups, _ = big
    four = soa.Groups(*[getattr(groups, k)[..., :4].copy() for k in GROUP_FIELDS])
    with bsa.Context(scalar_lanes=nodes.lanes - 4) as ctx:
        ctx.load_nodes(nodes, fit)
        ctx.load_groups(four)
        ctx.apply_group_deltas([(2, int(four.matched[2]) + 1, int(four.status_scheduled[2]), int(four.flags[2]))])
        ctx.load_groups(groups)
        back = ctx.read_groups()
        for k in GROUP_FIELDS:
            assert np.array_equal(getattr(back, k), getattr(groups, k)), k


def delta_blob_bytes(n_remove, n_insert, n_flags, lanes):
    """size of the blob bs_pods_apply stages for a delta: the index lists, then the inserted pods' arrays, each piece 16-byte aligned"""
    o = 0
    for piece in (n_remove * 4, n_insert * 4, n_flags * 4, n_flags,
                  n_insert * 4, n_insert * lanes * 8, n_insert * 4, n_insert * 4, n_insert * 8, n_insert):
        o = (o + piece + 15) & ~15
    return o + 16


def test_delta_staging_grows_between_two_applies(tiny, bsa, soa, orc):
    """h_dstage: two bs_pods_apply with no batch in between (the second waits for the stream); the first fits the buffer's first
    64 KiB, the second is the fewest inserted pods whose blob does not.  The batch over the patched queue equals the oracle."""
    nodes, fit, groups, pods, _, _ = tiny
    first_cap = 64 << 10
    n_ins = next(i for i in range(1, 1 << 16) if delta_blob_bytes(0, i, 0, nodes.lanes) > first_cap)
    rng = np.random.default_rng(7)
    small = dict(remove=np.arange(3, dtype=np.uint32), insert=pods.take(np.arange(3, 6)), insert_at=None)
    assert delta_blob_bytes(3, 3, 0, nodes.lanes) <= first_cap < delta_blob_bytes(0, n_ins, 0, nodes.lanes)
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        assert_batch_equal(ctx.batch(soa.STAGE_ALL), orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL), "before the deltas")
        cur = pods.patched(**small)
        large = dict(insert=cur.take(rng.integers(0, cur.p, n_ins)), insert_at=np.sort(rng.choice(cur.p + n_ins, n_ins, replace=False)).astype(np.uint32))
        ctx.apply_pods(**small)
        ctx.apply_pods(**large)
        cur = cur.patched(**large)
        assert_batch_equal(ctx.batch(soa.STAGE_ALL), orc.Sop(orc.Snapshot(nodes, fit), groups).batch(cur, soa.STAGE_ALL), "after two deltas")
        assert ctx.read_pods().equal(cur)


def test_node_request_staging_grows_between_two_assumes(tiny, bsa):
    """h_nstage: 4 node requests, then at once the fewest whose bytes exceed the buffer's first 16 KiB; bs_nodes_read is the host model."""
    nodes, fit, groups, pods, _, _ = tiny
    n_large = (16 << 10) // ctypes.sizeof(bsa.capi.NodeRequest) + 1
    assert n_large <= nodes.n
    cur = nodes.copy()

    def requests(idx, add):
        cur.requested[:4, idx] += add
        return [(int(n), cur.requested[:, n].tolist(), int(cur.requested_present[n])) for n in idx]

    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        ctx.assume_nodes(requests(np.arange(4), 1))
        ctx.assume_nodes(requests(np.arange(nodes.n - n_large, nodes.n), 2))
        req, pres = ctx.read_node_requests()
        assert np.array_equal(req, cur.requested) and np.array_equal(pres, cur.requested_present)


@pytest.fixture(scope="module")
def two_clusters(bsa, soa, orc):
    """the 96-pod queue over 64 nodes and over 4 096 nodes, with the oracle's batches"""
    out = []
    for n in (64, 4096):
        nodes, fit, groups, pods, _ = bsa.synth.make("tiny", "tail", nodes=n)
        out.append((nodes, fit, groups, pods, orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)))
    return out


@pytest.mark.parametrize("mode", ["read", "map"])
def test_result_staging_grows_with_the_node_count(mode, two_clusters, bsa, soa):
    """h_rstage (bs_batch_read's copies) and h_hout / h_hrows (BS_BATCH_HOST_RESULTS, read in place through bs_batch_map and copied
    out by bs_batch_read): one context, Filter over 64 nodes (one row word), then over 4 096 (64)."""
    nodes, fit, groups, pods, _ = two_clusters[0]
    with load_ctx(bsa, nodes, fit, groups, pods) as ctx:
        for nodes, fit, _, _, exp in two_clusters:
            ctx.load_nodes(nodes, fit)
            if mode == "read":
                assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp, f"{nodes.n} nodes")
                continue
            ctx.run(soa.STAGE_ALL | soa.BATCH_HOST_RESULTS)
            v = ctx.map_results()
            assert v["fl_rows"] is not None
            got = soa.BatchOut(*[v[k] for k in ("pf_code", "pf_first_k", "pf_leader", "fl_code", "fl_feasible")], None, v["group_admit"], v["group_ready"],
                               fl_slot=v["fl_slot"], fl_rows=v["fl_rows"], n=nodes.n)
            assert_batch_equal(got, exp, f"{nodes.n} nodes (mapped)", bitmap=False)
            assert np.array_equal(got.bitmap_from_rows(), exp.fl_bitmap), f"{nodes.n} nodes (mapped rows)"
            out = soa.BatchOut.alloc(pods.p, groups.g, nodes.n, bitmap=False, rows_cap=max(ctx.filter_rows_count(), 1))
            ctx.read(out=out)
            assert_batch_equal(out, exp, f"{nodes.n} nodes (read of the host results)", bitmap=False)
            assert np.array_equal(out.bitmap_from_rows(), exp.fl_bitmap), f"{nodes.n} nodes (rows read)"


# Device memory reaches a process in fragments of 2 MiB (the driver's large-page size): free memory that differs by more than one of them
# between two closes is memory a context kept.
GRANULE = 2 << 20


def test_fifty_contexts_leave_nothing_behind(tiny, bsa, soa):
    """50 x (create, load the 8-pod scene, one batch, destroy) in one process: every batch equals the oracle, and the device's free
    memory after the last destroy is within one allocation granule of what it was after the first.
    The observed difference is printed (run with -s); it has not been recorded here yet: no MI355X run of this loop exists so far."""
    nodes, fit, groups, _, pods8, exp8 = tiny
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    seen = []
    for it in range(50):
        with load_ctx(bsa, nodes, fit, groups, pods8) as ctx:
            assert_batch_equal(ctx.batch(soa.STAGE_ALL), exp8, f"context {it}")
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        seen.append(free.value)
    print(f"free bytes after close 1 / 50: {seen[0]} / {seen[-1]} (difference {seen[0] - seen[-1]}; largest over the loop {max(seen) - min(seen)})")
    assert abs(seen[0] - seen[-1]) <= GRANULE
