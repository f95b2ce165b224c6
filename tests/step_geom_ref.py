"""The launch geometry of the steady-state chain, restated in Python from run_fast as it stood BEFORE csrc/bs_step_geom.hpp existed (the
function that held the grid arithmetic, the ticket accounting and the launches in one piece).  tests/test_step_geom_cpu.py holds the header
against this; tests/preempt_commit_paths.geometry has the same role for the preemption geometry.

Every function takes numpy integer arrays (or scalars) that broadcast against each other and returns a dict of int64 arrays; booleans are
0 / 1.  The values of the walked grid stay far below 2^31, so the header's uint32 arithmetic and int64 here agree without wrap-around."""
import numpy as np

TBL_CHUNK = 256
STEP_SLOTS_MAX = 256
GATHER_DIRECT_BLOCKS = 8

# launch B's forms, as the header's enum counts them
FUSED, TWO_STREAMS, TRANSPOSED, SCAN_THEN_FILTER, PLAIN = range(5)


def i64(x):
    return np.asarray(x, dtype=np.int64)


def cdiv(a, b):
    return (i64(a) + b - 1) // b


def filter_role_blocks(waves, slot_tiles, W):
    return cdiv(np.minimum(i64(waves), i64(slot_tiles) * np.maximum(1, cdiv(W, 2))), 4)


def step_k(*, h_K, k_bound, kinfo_pending, step_a_form, dirs_ready):
    """k_step: prm.k_host when K is known, the bound for the whole-step form over a ready directory, else 0"""
    k_host = np.where(i64(kinfo_pending) != 0, 0, i64(h_K))
    return np.where(i64(kinfo_pending) == 0, k_host, np.where((i64(step_a_form) >= 3) & (i64(dirs_ready) != 0), i64(k_bound), 0))


def step_a_possible(k, *, P, M, S, step_a_on=1, no_fuse_final=0, collect_stats=0, enable_timing=0):
    k, nchunks = i64(k), np.maximum(1, cdiv(M, 256))
    return ((i64(step_a_on) != 0) & (i64(no_fuse_final) == 0) & (k > 0) & (k <= STEP_SLOTS_MAX) & (nchunks <= 64) & (i64(M) > 0) & (i64(P) > 0) &
            (i64(collect_stats) == 0) & (i64(enable_timing) < 2) & (i64(S) <= 4)).astype(np.int64)


def step_a_plan(K, *, P, N, M, step_a_form, step_shares, run_filter, dirs_ready, ranges_valid, nranges, kinfo_pending, filter_waves=8192,
                whole_bufs=1):
    K = i64(K)
    W = cdiv(N, 64)
    nchunks_m = np.maximum(1, cdiv(M, 256))
    nshares = np.maximum(1, np.minimum(i64(step_shares), cdiv(K, 8)))
    fblocks = np.where(i64(run_filter) != 0, cdiv(np.minimum(i64(filter_waves), cdiv(2 * K, 64) * np.maximum(1, cdiv(W, 2))), 4), 0)
    pb = np.where((i64(step_a_form) >= 2) & (i64(dirs_ready) != 0), cdiv(K, TBL_CHUNK), 0)
    nch_nodes = np.maximum(1, cdiv(N, 256))
    whole = ((i64(step_a_form) >= 3) & (pb != 0) & (nch_nodes <= 64) & (i64(whole_bufs) != 0)).astype(np.int64)
    nchunks = np.where(whole != 0, nch_nodes, nchunks_m)
    ranges = ((whole != 0) & (i64(ranges_valid) != 0) & (i64(nranges) != 0)).astype(np.int64)
    qb = np.where(ranges != 0, i64(nranges), cdiv(P, TBL_CHUNK))
    grid = qb + pb + nchunks * nshares + fblocks
    ready = ((i64(kinfo_pending) == 0) | (whole != 0)).astype(np.int64)
    return dict(ready=ready, whole=whole, ranges=ranges, qb=qb, pb=pb, nchunks=nchunks, nshares=nshares, fblocks=fblocks, grid=grid,
                launches=np.where(whole != 0, 1, 2),
                tk_pods=np.where(pb != 0, pb, qb),
                tk_tab=np.where(whole != 0, 0, nchunks),
                tk_p1=np.where(whole != 0, qb, 0),
                tk_done=np.where((whole != 0) & (qb > GATHER_DIRECT_BLOCKS), nchunks * nshares + fblocks, 0))


def launch_b_plan(*, P, N, M, S, h_K, kinfo_pending, tp_filter, run_filter, nranks, fused_fits=1, filter_waves=8192, filter_waves_env=0,
                  tp_share=0, tp_fwaves=0, tp_tmin=768, target_waves=8192, scan_share=0, no_fuse_final=0, no_nodew=0, have_nodew=1):
    W = cdiv(N, 64)
    h_K, tp_filter, run_filter = i64(h_K), i64(tp_filter), i64(run_filter)
    k_est = np.minimum(i64(P), np.where(i64(kinfo_pending) != 0, np.maximum(2 * h_K, 1024), np.maximum(h_K, 1)))
    tiles = cdiv(k_est, 64)
    throughput = tiles > 16
    node_words = (run_filter != 0) & throughput & (tp_filter >= 5) & (i64(no_nodew) == 0) & (i64(have_nodew) != 0)
    tiles2_min = i64(tp_tmin) * np.maximum(1, i64(nranks))
    nseg = np.where(i64(scan_share) != 0, i64(scan_share), 8)
    share_b = np.where(i64(tp_share) != 0, i64(tp_share), np.where(throughput, 2, 64))
    units = cdiv(2 * k_est, 64) * np.maximum(1, cdiv(W, 2))
    regime_waves = np.where(i64(tp_fwaves) != 0, i64(tp_fwaves), np.where(units >= 65536, np.maximum(i64(filter_waves), 16384), i64(filter_waves)))
    fw = np.where(throughput & (tp_filter >= 5) & (i64(filter_waves_env) == 0), regime_waves, i64(filter_waves))
    fblocks = np.where(run_filter != 0, cdiv(np.minimum(fw, units), 4), 0)

    def scan_grid(nsub):
        items = tiles * np.minimum(nseg if nsub == 4 else share_b, cdiv(M, 64))
        return np.maximum(1, np.minimum(cdiv(target_waves, 4), items if nsub == 4 else cdiv(items, 4)))

    fused_grid = scan_grid(4) + fblocks + cdiv(P, 256)
    fused = (tiles <= 16) & (i64(no_fuse_final) == 0) & (i64(fused_fits) != 0)
    scan_nsub = np.where(fused, 4, 1)
    scan_blocks = np.where(fused, scan_grid(4), scan_grid(1))
    split = (fblocks != 0) & throughput
    form = np.where(fused, FUSED,
                    np.where((tp_filter == 8) & split, TWO_STREAMS,
                             np.where((tp_filter >= 6) & split & (i64(S) <= 4), TRANSPOSED,
                                      np.where((tp_filter != 0) & split, SCAN_THEN_FILTER, PLAIN))))
    launches = np.where(fused, 2, np.where((form == TWO_STREAMS) | (form == SCAN_THEN_FILTER), 4, 3))
    return dict(form=form, throughput=throughput.astype(np.int64), node_words=node_words.astype(np.int64), tiles2_min=tiles2_min, nseg=nseg,
                share_b=share_b, scan_nsub=scan_nsub, scan_blocks=scan_blocks, fblocks=fblocks, filter_waves=fw, fused_grid=fused_grid,
                launches=launches, tiles=tiles)
