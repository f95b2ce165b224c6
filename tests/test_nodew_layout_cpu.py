"""CPU: the layout of the batch's node words (batch-scheduler_amd/csrc/bs_nodew_layout.hpp) on its own, compiled with g++.  The header is the index
arithmetic that ships: node_words_block (bs_fast.hpp), the lean Filter items (bs_filter_t.hpp), the allocation and the grid of launch A (bsched.hip)
all call it.  The driver walks every store the grid makes for a node count N — (block, wave, table) plus block 0's ref[] stores — exactly as the
kernel does, and reports what is wrong:

  bit 0  a store of table t outside [pair(t, 0), pair(t, W)), W = cdiv(N, 64)
  bit 1  a word w < W of some table written by no wave, or by more than one
  bit 2  one address written from two different sources, or ref[] inside a table
  bit 3  an address at or beyond the allocated size

THIS is the detector of the stray store the suite could not see (a wave of the last block without a single node wrote pair `stride` of its table =
pair 0 of the next table, racing with block 0's valid store): the GPU parity scenes of tests/test_gpu_nodew.py are a net, a race does not lose every
time.  The driver's second mode ignores the "does this wave store" predicate, which is the arithmetic as it was before the guard: it must collide for
exactly the N with N mod 256 in [1, 64] — that shows the walk sees the defect, and that the guard is what removes it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "batch-scheduler_amd", "csrc", "bs_nodew_layout.hpp")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>
#include "bs_nodew_layout.hpp"
using namespace bs;
// usage: drv <guard 0|1> N...   prints "N bits" per node count
static unsigned walk(uint32_t N, bool guard) {
  const uint32_t W = nodew_words(N), stride = nodew_stride(N);
  const size_t alloc = nodew_alloc_words(N);
  unsigned bad = 0;
  std::map<size_t, int> src;                         // address -> source id of its (one) writer
  std::vector<std::vector<int>> writers(kNodewTables, std::vector<int>(W, 0));
  auto store = [&](size_t addr, int id) {
    if (addr >= alloc) bad |= 8u;
    auto it = src.find(addr);
    if (it != src.end() && it->second != id) bad |= 4u;
    src[addr] = id;
  };
  int id = 0;
  for (uint32_t blk = 0; blk < nodew_blocks(N); ++blk)
    for (uint32_t wave = 0; wave < kNodewBlockThreads / 64u; ++wave) {
      const uint32_t w = nodew_wave_word(blk, wave * 64u);
      for (uint32_t lane = 1; lane < 64u; ++lane)
        if (nodew_wave_word(blk, wave * 64u + lane) != w) bad |= 1u;       // a wave is one 64-node block
      if (guard && !nodew_wave_stores(N, w)) continue;
      for (int t = 0; t < kNodewTables; ++t) {
        const size_t a = nodew_pair(stride, t, w);
        if (a < nodew_pair(stride, t, 0) || a + 1 >= nodew_pair(stride, t, 0) + 2u * W) bad |= 1u;
        if (w < W) writers[t][w]++;
        ++id;
        store(a, id);
        store(a + 1, id);
      }
    }
  for (int t = 0; t < kNodewTables; ++t)
    for (uint32_t w = 0; w < W; ++w)
      if (writers[t][w] != 1) bad |= 2u;
  // block 0, thread 0: ref[]
  for (int s = 0; s < kNodewLeaders; ++s) {
    for (int j = 0; j < 4; ++j) store(nodew_ref_lane(stride, s, j), ++id);
    store(nodew_ref_flags(stride, s), ++id);
  }
  // ref[] lies behind every pair a reader may fetch (the lean loop's loads run ahead into the two padding pairs of a table); tables do not overlap
  if (nodew_ref(stride) < nodew_pair(stride, kNodewTables - 1, 0) + 2u * stride) bad |= 4u;
  if (nodew_ref_flags(stride, kNodewLeaders - 1) >= alloc) bad |= 8u;
  for (int t = 0; t + 1 < kNodewTables; ++t)
    if (nodew_table(stride, t) + 2u * stride != nodew_table(stride, t + 1)) bad |= 4u;
  return bad;
}
int main(int argc, char** argv) {
  const bool guard = std::atoi(argv[1]) != 0;
  for (int i = 2; i < argc; ++i) {
    const uint32_t N = (uint32_t)std::strtoul(argv[i], nullptr, 10);
    std::printf("%u %u\n", N, walk(N, guard));
  }
  return 0;
}
"""

SIZES = list(range(1, 4097)) + [5000, 16384] + list(range(19999, 20066))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile bs_nodew_layout.hpp")
    d = tmp_path_factory.mktemp("nodew")
    src, exe = d / "drv.cpp", d / "drv"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-o", str(exe), str(src)], check=True)

    def run(sizes, guard):
        out = {}
        for a in range(0, len(sizes), 512):
            res = subprocess.run([str(exe), "1" if guard else "0", *map(str, sizes[a:a + 512])], check=True, capture_output=True, text=True).stdout
            for line in res.splitlines():
                n, bits = line.split()
                out[int(n)] = int(bits)
        assert sorted(out) == sorted(sizes)
        return out
    return run


def test_every_store_of_the_grid_lands_in_its_own_table(walk):
    bad = {n: bits for n, bits in walk(SIZES, True).items() if bits}
    assert not bad, f"node counts whose node-word stores collide or leave their table (N: bits): {dict(list(bad.items())[:16])} ({len(bad)} in all)"


def test_without_the_store_predicate_the_walk_fails_exactly_where_the_last_block_has_an_empty_wave_one_past_the_table(walk):
    """The arithmetic before the guard (every wave stores).  A wave of the last block without a node has w >= W.  For N mod 256 in [65, 192] such
    waves have w = W or W + 1: the two padding pairs of their OWN table — outside [0, W) (bit 0), but nobody else's.  For N mod 256 in [1, 64] wave 3
    has w = W + 2 = stride: pair 0 of the NEXT table (ref[0..1] from table 2), which block 0 writes in the same launch — a collision (bit 2).  That
    set, and no other, is where the shipped library could answer wrong."""
    res = walk(SIZES, False)
    collide = sorted(n for n, bits in res.items() if bits & 4)
    assert collide == [n for n in SIZES if 1 <= n % 256 <= 64]
    assert sorted(n for n, bits in res.items() if bits & 1) == [n for n in SIZES if 1 <= n % 256 <= 192]
    assert all(bits == 0 for n, bits in res.items() if not 1 <= n % 256 <= 192)
    assert not any(bits & 8 for bits in res.values())                      # (the stray pair still lies inside the allocation: nothing faulted, it was only wrong)
    assert all(bits & 2 == 0 for bits in res.values())                     # every word of every table still had its one writer


def test_header_has_no_hip_dependency():
    text = open(HDR).read()
    assert "hip_runtime" not in text and "#include \"" not in text
