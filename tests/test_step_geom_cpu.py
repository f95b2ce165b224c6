"""CPU: the launch geometry of the steady-state chain (batch-scheduler_amd/csrc/bs_step_geom.hpp) on its own, compiled with g++.  The header
is the arithmetic that ships: run_fast (bsched.hip) fills a StepIn, asks step_a_plan / launch_b_plan, launches what the plan says and advances
the tickets by what the plan says.  A ticket advance that is not the number of blocks that add to the counter is a launch that waits inside
itself for ever, so the rules between grid and tickets are checked here, where no GPU can hang.

The driver walks the full product of the grid below, slice by slice of (P, N, M), and reports per slice

  bits    rules some point of the slice breaks (0 = none), see RULES
  sums    per field of the plans, the sum over the slice's points of (2 i + 1) * value (i = the point's index in the slice, mod 2^64)

which the Python restatement (tests/step_geom_ref.py, written from run_fast as it stood before the header) has to reproduce field by field.
The driver has its own main, so it can also be built with -fsanitize=address,undefined as a stand-alone program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import step_geom_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "batch-scheduler_amd", "csrc")
HDR = os.path.join(CSRC, "bs_step_geom.hpp")

RULES = {
    0: "grid != qb + pb + nchunks * nshares + fblocks",
    1: "a step the one-launch form can take has qb, nchunks or nshares < 1",
    2: "fblocks > cdiv(filter_waves, 4)",
    3: "a ticket advance is not the one the header's comment states",
    4: "whole without cdiv(N, 256) <= 64 and pb > 0",
    5: "launches == 1 is not the same as whole",
    6: "launch B fused with more than 16 tiles",
    7: "launch B transposed in one launch with S > 4",
    8: "node_words without Filter, tp_filter >= 5 and the throughput regime",
    9: "launch B: launches is not 2 when fused, 4 for the two split forms, 3 otherwise",
    10: "effective Filter waves differ from the context's outside (throughput, tp_filter >= 5, no BS_FILTER_WAVES)",
    11: "launch B fused although the caller said its grid does not fit",
}

A_FIELDS = ["ready", "whole", "ranges", "qb", "pb", "nchunks", "nshares", "fblocks", "grid", "launches", "tk_pods", "tk_tab", "tk_p1", "tk_done"]
B_FIELDS = ["form", "throughput", "node_words", "tiles2_min", "nseg", "share_b", "scan_nsub", "scan_blocks", "fblocks", "filter_waves", "fused_grid", "launches"]
# the inputs of one point, in the order the driver's `one` mode reads them
IN_FIELDS = ["P", "N", "M", "S", "h_K", "k_bound", "kinfo_pending", "step_a_form", "step_shares", "step_a_on", "filter_waves", "filter_waves_env",
             "tp_filter", "tp_share", "tp_fwaves", "tp_tmin", "target_waves", "scan_share", "nranks", "run_filter", "dirs_ready", "ranges_valid",
             "nranges", "whole_bufs", "no_fuse_final", "no_nodew", "have_nodew", "collect_stats", "enable_timing"]

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "bs_step_geom.hpp"
using namespace bs;
typedef unsigned long long u64;
// usage: drv walk                 prints "P N M bits sums..." per slice of the grid (the tables below)
//        drv one v...             prints "K possible A-fields B-fields(fits) B-fields(does not fit)" per point of 29 inputs
static const uint32_t Ps[] = {0, 1, 255, 256, 257, 5000};
static const uint32_t Ns[] = {1, 63, 64, 65, 255, 256, 257, 16384, 16385, 20000};
static const uint32_t Ms[] = {0, 1, 256, 257, 0xFFFFFFFFu /* = N */};
static const uint32_t Ks[] = {1, 7, 8, 9, 64, 255, 256, 257, 1024, 1025, 5000};
static const uint32_t Shares[] = {1, 8, 32};
static const uint32_t Ss[] = {1, 4, 5, 12};
static const uint32_t Ranks[] = {1, 8};
template <class T, size_t n> constexpr size_t len(const T (&)[n]) { return n; }

static StepIn base() {
  StepIn in{};
  in.G = 16; in.step_a_on = true; in.filter_waves = 8192; in.tp_tmin = 768; in.target_waves = 8192; in.whole_bufs = true; in.have_nodew = true;
  return in;
}
static size_t fields_a(const StepAPlan& p, u64* v) {
  const u64 f[] = {p.ready, p.whole, p.ranges, p.qb, p.pb, p.nchunks, p.nshares, p.fblocks, p.grid, p.launches, p.tk_pods, p.tk_tab, p.tk_p1, p.tk_done};
  for (size_t i = 0; i < len(f); ++i) v[i] = f[i];
  return len(f);
}
static size_t fields_b(const LaunchBPlan& p, u64* v) {
  const u64 f[] = {(u64)p.form, p.throughput, p.node_words, p.tiles2_min, p.nseg, p.share_b, p.scan_nsub, p.scan_blocks, p.fblocks, p.filter_waves,
                   p.fused_grid, p.launches};
  for (size_t i = 0; i < len(f); ++i) v[i] = f[i];
  return len(f);
}
static unsigned rules_a(const StepIn& in, const StepAPlan& p, bool possible) {
  unsigned bad = 0;
  if (p.grid != p.qb + p.pb + p.nchunks * p.nshares + p.fblocks) bad |= 1u << 0;
  if (possible && (p.qb < 1 || p.nchunks < 1 || p.nshares < 1)) bad |= 1u << 1;
  if (p.fblocks > cdiv(in.filter_waves, 4)) bad |= 1u << 2;
  if (p.tk_pods != (p.pb ? p.pb : p.qb) || p.tk_tab != (p.whole ? 0u : p.nchunks) || p.tk_p1 != (p.whole ? p.qb : 0u) ||
      p.tk_done != ((p.whole && p.qb > kGatherDirectBlocks) ? p.nchunks * p.nshares + p.fblocks : 0u)) bad |= 1u << 3;
  if (p.whole && !(cdiv(in.N, 256) <= 64 && p.pb > 0)) bad |= 1u << 4;
  if ((p.launches == 1) != p.whole || p.launches < 1 || p.launches > 2) bad |= 1u << 5;
  return bad;
}
static unsigned rules_b(const StepIn& in, const LaunchBPlan& p, bool fits) {
  unsigned bad = 0;
  const uint32_t k_est = geom_min(in.P, in.kinfo_pending ? geom_max(2 * in.h_K, 1024u) : geom_max(in.h_K, 1u));
  const bool tp = cdiv(k_est, 64) > 16;
  const bool split = p.form == LaunchB::kTwoStreams || p.form == LaunchB::kScanThenFilter;
  if (p.form == LaunchB::kFused && cdiv(k_est, 64) > 16) bad |= 1u << 6;
  if (p.form == LaunchB::kTransposed && in.S > 4) bad |= 1u << 7;
  if (p.node_words && !(in.run_filter && in.tp_filter >= 5 && tp)) bad |= 1u << 8;
  if (p.launches != (p.form == LaunchB::kFused ? 2u : split ? 4u : 3u)) bad |= 1u << 9;
  if (p.filter_waves != in.filter_waves && !(tp && in.tp_filter >= 5 && !in.filter_waves_env)) bad |= 1u << 10;
  if (!fits && p.form == LaunchB::kFused) bad |= 1u << 11;
  return bad;
}
int main(int argc, char** argv) {
  u64 v[64];
  if (argv[1][0] == 'o') {
    for (int i = 2; i + 28 < argc; i += 29) {
      uint32_t a[29];
      for (int j = 0; j < 29; ++j) a[j] = (uint32_t)std::strtoul(argv[i + j], nullptr, 10);
      StepIn in{};
      in.P = a[0]; in.N = a[1]; in.M = a[2]; in.S = a[3]; in.W = cdiv(in.N, 64); in.G = 16;
      in.h_K = a[4]; in.k_bound = a[5]; in.kinfo_pending = a[6]; in.k_host = in.kinfo_pending ? 0u : in.h_K;
      in.step_a_form = a[7]; in.step_shares = a[8]; in.step_a_on = a[9]; in.filter_waves = a[10]; in.filter_waves_env = a[11];
      in.tp_filter = a[12]; in.tp_share = a[13]; in.tp_fwaves = a[14]; in.tp_tmin = a[15]; in.target_waves = a[16]; in.scan_share = a[17];
      in.nranks = a[18]; in.run_filter = a[19]; in.dirs_ready = a[20]; in.ranges_valid = a[21]; in.nranges = a[22]; in.whole_bufs = a[23];
      in.no_fuse_final = a[24]; in.no_nodew = a[25]; in.have_nodew = a[26]; in.collect_stats = a[27]; in.enable_timing = (int)a[28];
      const uint32_t K = step_k(in);
      const bool possible = step_a_possible(in, K, table_chunks(in.M));
      size_t n = fields_a(step_a_plan(in, K), v);
      n += fields_b(launch_b_plan(in, true), v + n);
      n += fields_b(launch_b_plan(in, false), v + n);
      std::printf("%u %u", K, possible ? 1u : 0u);
      for (size_t j = 0; j < n; ++j) std::printf(" %llu", v[j]);
      std::printf("\n");
    }
    return 0;
  }
  for (uint32_t P : Ps) for (uint32_t N : Ns) for (uint32_t Mv : Ms) {
    StepIn in = base();
    in.P = P; in.N = N; in.M = Mv == 0xFFFFFFFFu ? N : Mv; in.W = cdiv(N, 64);
    in.nranges = cdiv(P, 200);
    unsigned bad = 0;
    u64 sum[64] = {0}, idx = 0;
    size_t nf = 0;
    for (uint32_t K : Ks) for (uint32_t form = 0; form < 4; ++form) for (uint32_t sh : Shares) for (uint32_t tp = 0; tp < 9; ++tp) for (uint32_t S : Ss)
    for (int rf = 0; rf < 2; ++rf) for (int dr = 0; dr < 2; ++dr) for (int rg = 0; rg < 2; ++rg) for (int kp = 0; kp < 2; ++kp) for (uint32_t nr : Ranks) {
      in.h_K = K; in.k_bound = K; in.kinfo_pending = kp; in.k_host = kp ? 0u : K;
      in.step_a_form = form; in.step_shares = sh; in.tp_filter = tp; in.S = S; in.run_filter = rf; in.dirs_ready = dr; in.ranges_valid = rg; in.nranks = nr;
      const uint32_t Ks_ = step_k(in);
      const bool possible = step_a_possible(in, Ks_, table_chunks(in.M));
      const StepAPlan pa = step_a_plan(in, Ks_);
      const LaunchBPlan b1 = launch_b_plan(in, true), b0 = launch_b_plan(in, false);
      bad |= rules_a(in, pa, possible) | rules_b(in, b1, true) | rules_b(in, b0, false);
      v[0] = Ks_; v[1] = possible;
      nf = 2 + fields_a(pa, v + 2);
      nf += fields_b(b1, v + nf);
      nf += fields_b(b0, v + nf);
      const u64 w = 2 * idx + 1;
      for (size_t j = 0; j < nf; ++j) sum[j] += w * v[j];
      ++idx;
    }
    std::printf("%u %u %u %u", P, N, in.M, bad);
    for (size_t j = 0; j < nf; ++j) std::printf(" %llu", sum[j]);
    std::printf("\n");
  }
  return 0;
}
"""

PS = [0, 1, 255, 256, 257, 5000]
NS = [1, 63, 64, 65, 255, 256, 257, 16384, 16385, 20000]
MS = [0, 1, 256, 257, None]                # None = N
# the axes inside a slice, outermost first (the driver's loop order)
AXES = [("K", [1, 7, 8, 9, 64, 255, 256, 257, 1024, 1025, 5000]), ("step_a_form", [0, 1, 2, 3]), ("step_shares", [1, 8, 32]), ("tp_filter", list(range(9))),
        ("S", [1, 4, 5, 12]), ("run_filter", [0, 1]), ("dirs_ready", [0, 1]), ("ranges_valid", [0, 1]), ("kinfo_pending", [0, 1]), ("nranks", [1, 8])]


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile bs_step_geom.hpp")
    d = tmp_path_factory.mktemp("sgeom")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)], check=True)

    def run(*args):
        res = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout
        return [tuple(int(x) for x in line.split()) for line in res.splitlines()]
    return run


@pytest.fixture(scope="module")
def walked(drv):
    out = {(p, n, m): (bits, sums) for p, n, m, bits, *sums in drv("walk")}
    assert len(out) == len({(p, n, n if m is None else m) for p in PS for n in NS for m in MS})
    return out


def _axes():
    shape = [len(v) for _, v in AXES]
    ax = {}
    for i, (name, vals) in enumerate(AXES):
        s = [1] * len(AXES)
        s[i] = len(vals)
        ax[name] = np.array(vals, dtype=np.int64).reshape(s)
    w = (2 * np.arange(int(np.prod(shape)), dtype=np.uint64) + 1).reshape(shape)
    return ax, w


def _weighted(w, val, cache):
    """sum of w * val (mod 2^64) over the slice; val broadcasts against w, so w is first summed over the axes val does not vary along"""
    shape = (1,) * (w.ndim - val.ndim) + val.shape
    if shape not in cache:
        cache[shape] = w.sum(axis=tuple(i for i, n in enumerate(shape) if n == 1), keepdims=True, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int((cache[shape] * val.reshape(shape).astype(np.uint64)).sum(dtype=np.uint64))


def _restated(P, N, M, ax):
    """the restatement's fields for one slice, in the driver's order; values broadcast over the slice's axes"""
    kw = dict(P=P, N=N, M=M)
    K = ref.step_k(h_K=ax["K"], k_bound=ax["K"], kinfo_pending=ax["kinfo_pending"], step_a_form=ax["step_a_form"], dirs_ready=ax["dirs_ready"])
    possible = ref.step_a_possible(K, P=P, M=M, S=ax["S"])
    a = ref.step_a_plan(K, **kw, step_a_form=ax["step_a_form"], step_shares=ax["step_shares"], run_filter=ax["run_filter"], dirs_ready=ax["dirs_ready"],
                        ranges_valid=ax["ranges_valid"], nranges=ref.cdiv(P, 200), kinfo_pending=ax["kinfo_pending"])
    bkw = dict(**kw, S=ax["S"], h_K=ax["K"], kinfo_pending=ax["kinfo_pending"], tp_filter=ax["tp_filter"], run_filter=ax["run_filter"], nranks=ax["nranks"])
    b1, b0 = ref.launch_b_plan(**bkw, fused_fits=1), ref.launch_b_plan(**bkw, fused_fits=0)
    return K, possible, a, b1, b0


def test_header_equals_the_restatement_and_keeps_the_rules_over_the_grid(walked):
    ax, w = _axes()
    wsum = {}
    names = ["K", "possible"] + ["A." + f for f in A_FIELDS] + ["B." + f for f in B_FIELDS] + ["B'." + f for f in B_FIELDS]
    for (P, N, M), (bits, sums) in walked.items():
        assert bits == 0, f"P={P} N={N} M={M}: " + "; ".join(t for b, t in RULES.items() if bits >> b & 1)
        K, possible, a, b1, b0 = _restated(P, N, M, ax)
        vals = [K, possible] + [a[f] for f in A_FIELDS] + [b1[f] for f in B_FIELDS] + [b0[f] for f in B_FIELDS]
        assert len(vals) == len(sums)
        for name, val, got in zip(names, vals, sums):
            want = _weighted(w, np.asarray(val), wsum)
            assert want == got, f"P={P} N={N} M={M}: {name} of bs_step_geom.hpp differs from tests/step_geom_ref.py at some point of the slice"
        # the same rules on the restatement's own numbers (a checksum match alone would not say WHICH rule a changed header broke)
        assert np.all(a["grid"] == a["qb"] + a["pb"] + a["nchunks"] * a["nshares"] + a["fblocks"])
        taken = np.broadcast_to(possible != 0, w.shape)
        for part in ("qb", "nchunks", "nshares"):
            assert np.all(np.broadcast_to(a[part], w.shape)[taken] >= 1), part
        assert np.all(a["fblocks"] <= 8192 // 4)
        assert np.all(a["tk_pods"] == np.where(a["pb"] != 0, a["pb"], a["qb"]))
        assert np.all(a["tk_tab"] == np.where(a["whole"] != 0, 0, a["nchunks"]))
        assert np.all(a["tk_p1"] == np.where(a["whole"] != 0, a["qb"], 0))
        assert np.all(a["tk_done"] == np.where((a["whole"] != 0) & (a["qb"] > ref.GATHER_DIRECT_BLOCKS), a["nchunks"] * a["nshares"] + a["fblocks"], 0))
        assert np.all((a["whole"] == 0) | ((ref.cdiv(N, 256) <= 64) & (a["pb"] > 0)))
        assert np.all((a["launches"] == 1) == (a["whole"] != 0))
        for b, fits in ((b1, True), (b0, False)):
            split = (b["form"] == ref.TWO_STREAMS) | (b["form"] == ref.SCAN_THEN_FILTER)
            assert np.all((b["form"] != ref.FUSED) | (b["tiles"] <= 16))
            assert fits or np.all(b["form"] != ref.FUSED)
            assert np.all((b["form"] != ref.TRANSPOSED) | (ax["S"] <= 4))
            assert np.all((b["node_words"] == 0) | ((ax["run_filter"] != 0) & (ax["tp_filter"] >= 5) & (b["throughput"] != 0)))
            assert np.all(b["launches"] == np.where(b["form"] == ref.FUSED, 2, np.where(split, 4, 3)))
            assert np.all((b["filter_waves"] == 8192) | ((b["throughput"] != 0) & (ax["tp_filter"] >= 5)))


def test_the_grid_reaches_every_form_and_both_sides_of_the_chunk_limit(walked):
    """the rules above would hold vacuously over a grid that never took the one-launch forms or never left the latency regime"""
    ax, w = _axes()
    _, possible, a, b1, b0 = _restated(5000, 16384, 16384, ax)
    assert np.any((a["whole"] != 0) & (possible != 0)) and np.any((a["tk_done"] != 0) & (possible != 0))
    assert np.any((a["whole"] == 0) & (a["pb"] != 0) & (possible != 0)) and np.any((a["pb"] == 0) & (possible != 0))
    assert np.any(a["ranges"] != 0) and np.any((a["whole"] != 0) & (a["ranges"] == 0))
    assert sorted(np.unique(b1["form"])) == [ref.FUSED, ref.TWO_STREAMS, ref.TRANSPOSED, ref.SCAN_THEN_FILTER, ref.PLAIN]
    assert np.any(b1["node_words"] != 0) and np.any(b1["form"] != b0["form"])
    # N = 16384 is the last node count of the whole-step form, 16385 the first without it; M = N = 16385 leaves the one-launch forms altogether
    _, possible, a, _, _ = _restated(5000, 16385, 256, ax)
    assert not np.any(a["whole"] != 0) and np.any(possible != 0)
    _, possible, _, _, _ = _restated(5000, 16385, 16385, ax)
    assert not np.any(possible != 0)
    _, _, a, _, _ = _restated(256, 256, 256, ax)
    assert not np.any(a["tk_done"] != 0), "a queue of one pod block gathers directly: no kTkDone advance"


def test_switches_the_grid_leaves_at_their_defaults(drv):
    """BS_FILTER_WAVES, BS_TP_SHARE, BS_TP_FWAVES, the scan-share override, BS_NO_FUSE_FINAL, BS_NO_NODEW, BS_STEP_A=0, stats and timing, missing
    record buffers: seeded random points, header against restatement, field by field"""
    rng = np.random.default_rng(20240611)
    n = 3000
    pick = lambda vals: rng.choice(np.array(vals, dtype=np.int64), size=n)
    flag = lambda p: (rng.random(n) < p).astype(np.int64)
    v = dict(P=pick(PS + [70000]), N=pick(NS + [100000]), M=pick([0, 1, 63, 64, 256, 257, 16384, 16385]), S=pick([0, 1, 4, 5, 12]),
             h_K=pick([0, 1, 7, 8, 9, 64, 255, 256, 257, 1024, 1025, 5000, 40000]), k_bound=pick([0, 1, 200, 256, 257, 5000]), kinfo_pending=flag(0.3),
             step_a_form=pick([0, 1, 2, 3]), step_shares=pick([1, 2, 8, 32]), step_a_on=1 - flag(0.1), filter_waves=pick([1, 4, 100, 8192, 16384, 40000]),
             filter_waves_env=flag(0.3), tp_filter=pick(list(range(9))), tp_share=pick([0, 0, 1, 2, 8, 64]), tp_fwaves=pick([0, 0, 1024, 32768]),
             tp_tmin=pick([1, 768]), target_waves=pick([4, 1000, 8192]), scan_share=pick([0, 0, 1, 4, 64]), nranks=pick([0, 1, 8]), run_filter=flag(0.7),
             dirs_ready=flag(0.7), ranges_valid=flag(0.5), nranges=pick([0, 1, 9, 30]), whole_bufs=1 - flag(0.1), no_fuse_final=flag(0.1),
             no_nodew=flag(0.2), have_nodew=flag(0.8), collect_stats=flag(0.1), enable_timing=pick([0, 0, 1, 2]))
    rows = np.stack([v[f] for f in IN_FIELDS], axis=1)
    got = []
    for a in range(0, n, 200):
        got += drv("one", *rows[a:a + 200].ravel())
    assert len(got) == n
    K = ref.step_k(h_K=v["h_K"], k_bound=v["k_bound"], kinfo_pending=v["kinfo_pending"], step_a_form=v["step_a_form"], dirs_ready=v["dirs_ready"])
    possible = ref.step_a_possible(K, **{f: v[f] for f in ("P", "M", "S", "step_a_on", "no_fuse_final", "collect_stats", "enable_timing")})
    a = ref.step_a_plan(K, **{f: v[f] for f in ("P", "N", "M", "step_a_form", "step_shares", "run_filter", "dirs_ready", "ranges_valid", "nranges",
                                                 "kinfo_pending", "filter_waves", "whole_bufs")})
    bkw = {f: v[f] for f in ("P", "N", "M", "S", "h_K", "kinfo_pending", "tp_filter", "run_filter", "nranks", "filter_waves", "filter_waves_env", "tp_share",
                             "tp_fwaves", "tp_tmin", "target_waves", "scan_share", "no_fuse_final", "no_nodew", "have_nodew")}
    b1, b0 = ref.launch_b_plan(**bkw, fused_fits=1), ref.launch_b_plan(**bkw, fused_fits=0)
    want = np.stack([np.broadcast_to(x, (n,)) for x in [K, possible] + [a[f] for f in A_FIELDS] + [b1[f] for f in B_FIELDS] + [b0[f] for f in B_FIELDS]], axis=1)
    names = ["K", "possible"] + ["A." + f for f in A_FIELDS] + ["B." + f for f in B_FIELDS] + ["B'." + f for f in B_FIELDS]
    diff = np.argwhere(want != np.array(got, dtype=np.int64))
    assert diff.size == 0, f"point {dict(zip(IN_FIELDS, rows[diff[0][0]]))}: {names[diff[0][1]]} is {got[diff[0][0]][diff[0][1]]}, restated {want[tuple(diff[0])]}"
    assert np.any(possible != 0) and np.any(b1["filter_waves"] != v["filter_waves"])


def test_header_has_no_hip_dependency():
    text = open(HDR).read()
    assert "hip_runtime" not in text and "#include \"" not in text and "__global__" not in text


def test_run_fast_keeps_no_second_copy():
    text = open(os.path.join(CSRC, "bsched.hip")).read()
    assert "FwGuard" not in text
    assert len(re.findall(r"hipLaunchKernelGGL\(\s*k_fast_commit\b", text)) == 1
    assert "h_info.p)[" not in text and not re.search(r"h_info\.p\s*\+\s*\d", text)
    assert "step_a_plan(" in text and "launch_b_plan(" in text and "filter_blocks(" in text
    # the Filter role's block count is written in the header only
    for f in os.listdir(CSRC):
        if f != "bs_step_geom.hpp":
            assert not re.search(r"filter_waves,[^;\n]*cdiv\(W, 2\)", open(os.path.join(CSRC, f)).read()), f
