"""CPU: the launch geometry of the preemption search (batch-scheduler_amd/csrc/bs_preempt_geom.hpp) on its own, compiled with g++.  The
header is the arithmetic that ships: bs_preempt_run and bs_preempt_commit (tu_preempt.hip) both call preempt_geom().  The driver walks every
(N, tiles) of the grid below and reports, per node count N:

  bit 0  the chunks do not cover [0, N) exactly: not (nchunks - 1) * chunk_nodes < N <= nchunks * chunk_nodes (N > 0)
  bit 1  nchunks < 1 or chunk_nodes < 1
  bit 2  the spill of k_pc_resolve's rescan list is reachable for a 512-thread workgroup: nchunks > 512 and 4 * 513 <= 64 * tiles
  bit 3  the same for a 256-thread workgroup (12 scalar lanes)

and a checksum of (nchunks, chunk_nodes) over all tile counts, which the Python restatement (tests/preempt_commit_paths.geometry, what the
oracle-side classifier takes its geometry from) has to reproduce.  A slot lists a chunk for a rescan only when the kPcK = 4 recorded nodes
of it are dirty, a call dirties at most count <= 64 * tiles nodes, so T + 1 listed chunks need nchunks > T and 4 (T + 1) <= 64 tiles: bits
2 and 3 say that the shipped numbers make the spill unreachable.  Whoever retunes kPreemptWaves and sees them set has made the spill path
production code (it is tested through BS_TEST_PC_CHUNK_NODES by tests/test_gpu_preempt_commit_chunks.py either way)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import preempt_commit_paths as paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "batch-scheduler_amd", "csrc", "bs_preempt_geom.hpp")
ABI = os.path.join(ROOT, "include", "bsched.h")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "bs_preempt_geom.hpp"
using namespace bs;
// usage: drv walk <max tiles> N...          prints "N bits checksum" per node count (all tile counts 1..max, hook unset)
//        drv one <N> <count> <forced>       prints "tiles nchunks chunk_nodes" of preempt_geom(N, count, forced)
static bool spill(const PreemptGeom& g, uint32_t T) { return g.nchunks > T && 4ull * (T + 1ull) <= 64ull * g.tiles; }
int main(int argc, char** argv) {
  if (argv[1][0] == 'o') {
    for (int i = 2; i + 2 < argc; i += 3) {
      const PreemptGeom g = preempt_geom((uint32_t)std::strtoul(argv[i], nullptr, 10), (uint32_t)std::strtoul(argv[i + 1], nullptr, 10),
                                         (uint32_t)std::strtoul(argv[i + 2], nullptr, 10));
      std::printf("%u %u %u\n", g.tiles, g.nchunks, g.chunk_nodes);
    }
    return 0;
  }
  const uint32_t tmax = (uint32_t)std::strtoul(argv[2], nullptr, 10);
  for (int i = 3; i < argc; ++i) {
    const uint32_t N = (uint32_t)std::strtoul(argv[i], nullptr, 10);
    unsigned bad = 0;
    unsigned long long sum = 0;
    for (uint32_t t = 1; t <= tmax; ++t) {
      const PreemptGeom g = preempt_geom_tiles(N, t);
      if (g.tiles != t) bad |= 2u;
      if (N > 0 && !((unsigned long long)(g.nchunks - 1u) * g.chunk_nodes < N && N <= (unsigned long long)g.nchunks * g.chunk_nodes)) bad |= 1u;
      if (g.nchunks < 1u || g.chunk_nodes < 1u) bad |= 2u;
      if (spill(g, 512u)) bad |= 4u;
      if (spill(g, 256u)) bad |= 8u;
      sum += ((unsigned long long)g.nchunks * 0x9E3779B97F4A7C15ull + g.chunk_nodes) * (2ull * t + 1ull);
    }
    std::printf("%u %u %llu\n", N, bad, sum);
  }
  return 0;
}
"""

SIZES = list(range(0, 5001)) + [16384, 20000, 65536]


def _preempt_max() -> int:
    m = re.search(r"#define\s+BS_PREEMPT_MAX\s+\(1u\s*<<\s*(\d+)\)", open(ABI).read())
    assert m, "BS_PREEMPT_MAX not found in include/bsched.h"
    return 1 << int(m.group(1))


TMAX = _preempt_max() // 64


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile bs_preempt_geom.hpp")
    d = tmp_path_factory.mktemp("pgeom")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-o", str(exe), str(src)], check=True)

    def run(*args):
        res = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout
        return [tuple(int(x) for x in line.split()) for line in res.splitlines()]
    return run


@pytest.fixture(scope="module")
def walked(drv):
    out = {}
    for a in range(0, len(SIZES), 1024):
        for n, bits, chk in drv("walk", TMAX, *SIZES[a:a + 1024]):
            out[n] = (bits, chk)
    assert sorted(out) == sorted(SIZES)
    return out


def test_chunks_cover_the_node_list_and_the_rescan_list_cannot_spill_as_shipped(walked):
    assert TMAX == 16384
    bad = {n: bits for n, (bits, _) in walked.items() if bits}
    assert not bad, f"node counts whose geometry breaks a rule for some tile count (N: bits, see the module docstring): {dict(list(bad.items())[:16])}"


def test_python_restatement_equals_the_header_over_the_grid(walked):
    t = np.arange(1, TMAX + 1, dtype=np.int64)
    w = (2 * t + 1).astype(np.uint64)
    for n in SIZES:
        tiles, nch, cn = paths.geometry(n, tiles=t)
        assert np.array_equal(tiles, t)
        with np.errstate(over="ignore"):
            chk = int(((nch.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + cn.astype(np.uint64)) * w).sum(dtype=np.uint64))
        assert chk == walked[n][1], f"N={n}: tests/preempt_commit_paths.geometry differs from bs_preempt_geom.hpp for some tile count"
        # the same rules on the restatement's own numbers (a checksum match alone would not say WHICH rule a retuned header broke)
        assert np.all(nch >= 1) and np.all(cn >= 1)
        if n:
            assert np.all((nch - 1) * cn < n) and np.all(n <= nch * cn)
        for T in (512, 256):
            assert np.all((nch <= T) | (4 * (T + 1) > 64 * t)), f"N={n}, T={T}: the rescan list's spill is reachable under the shipped geometry"


def test_the_spill_rule_is_no_tautology():
    """four times the waves of the first launch would make the spill reachable: the rule above can fail"""
    t = np.arange(1, TMAX + 1, dtype=np.int64)
    _, nch, _ = paths.geometry(20000, tiles=t, waves=4 * paths.PREEMPT_WAVES)
    assert np.any((nch > 256) & (4 * 257 <= 64 * t))
    _, nch, _ = paths.geometry(20000, tiles=t)
    assert not np.any((nch > 256) & (4 * 257 <= 64 * t))


def test_forced_chunk_nodes_is_clamped_and_yields_to_the_grid_limit(drv):
    cases = []
    for n in (0, 1, 2, 5, 63, 64, 65, 257, 300, 1400, 2703, 20000, 65535, 65536, 65537, 200000, 1 << 20):
        for count in (1, 64, 65, 4096, 70000, 1 << 20):
            for forced in (0, 1, 2, 3, 4, 5, 64, n, n + 1, 1 << 31):
                cases.append((n, count, forced))
    got = []
    for a in range(0, len(cases), 300):
        got += drv("one", *[x for c in cases[a:a + 300] for x in c])
    assert len(got) == len(cases)
    for (n, count, forced), g in zip(cases, got):
        assert g == paths.geometry(n, count=count, forced=forced), (n, count, forced)
        tiles, nch, cn = g
        assert tiles == paths.cdiv(count, 64) and nch >= 1 and cn >= 1 and nch <= paths.GRID_Y_MAX
        if n:
            assert (nch - 1) * cn < n <= nch * cn
        shipped = paths.geometry(n, count=count)
        if forced == 0:
            assert g == shipped
        elif paths.cdiv(n, min(max(forced, 1), max(n, 1))) <= paths.GRID_Y_MAX:
            assert cn == min(forced, max(n, 1)) and nch == max(1, paths.cdiv(n, cn))
        else:
            assert g == shipped, "a forced value beyond the grid's y limit is ignored"
    # the shipped geometry of the scenes the bit-exact GPU tests use (tests/test_gpu_preempt_commit_chunks.py quotes these)
    assert [paths.geometry(n, count=q)[2] for n, q in ((400, 4096), (320, 4096), (257, 8192), (20000, 256), (640, 2048))] == [7, 5, 9, 20, 5]


def test_header_has_no_hip_dependency():
    text = open(HDR).read()
    assert "hip_runtime" not in text and "#include \"" not in text
