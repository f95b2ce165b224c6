"""CPU tests of bs_seq_run_scored's rule (include/bsched.h, rule P / D7): the object-level model tests/seq_scored_ref.py with zero weights
against the object replay of the plain pass (the full comparison, every scene), rule P stated a second time as a numpy table and a third
time by csrc/bs_seq_score.hpp compiled alone under the sanitizers, the hand-computed answers (tests/golden/seq_scored_hand_kats.json), the
non-vacuity of the scene set the GPU tests run (every hazard letter, with the scene that first shows it), and where the new kernels sit in
the build.  No GPU: nothing here creates a context."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import seq_obj_replay as sor
import seq_scored_ref as ssr
import seq_scored_scenes as sss

bsa = importlib.import_module("batch-scheduler_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
KEYS = ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods", "last_permitted", "matched", "status_scheduled", "latch", "closed",
        "denied")


# ---- P2: with zero weights the model is the plain pass ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", ["prefilter", "filter", "filter+deny"])
@pytest.mark.parametrize("seed", sss.SEEDS)
def test_zero_weights_are_the_object_replay(seed, stages):
    sc = sss.filter_scene(seed) if stages != "prefilter" and seed % 2 else sss.make(seed)
    kw = dict(run_filter=stages != "prefilter", filter_deny=stages == "filter+deny", scalar_names=sc["names"])
    got, plain = ssr.replay(sc, (0, 0, 0), **kw), sor.replay(sc, **kw)
    for k in KEYS:
        assert got[k] == plain[k], (seed, k)
    assert all(t == 0 for t in got["total"])
    assert sum(got["hazards"][c] for c in "acef") == 0, got["hazards"]
    for info_a, info_b in zip(got["op"].nodes, plain["op"].nodes):
        assert info_a.requested == info_b.requested and info_a.pod_count == info_b.pod_count


# ---- rule P three times --------------------------------------------------------------------------------------------------------------------------
def table(A0, R0, A1, R1, weights):
    """rule P over arrays of nodes (int64 columns) -> (least, most, balanced, total); masked lanes compute on (A, R) = (1, 0)"""
    def lane(A, R):
        dom = (A > 0) & (A < (1 << 53)) & (R >= 0) & (R <= A)
        a, r = np.where(dom, A, 1), np.where(dom, R, 0)
        return np.where(dom, ((a - r) * 100) // a, 0), np.where(dom, (r * 100) // a, 0), np.where(dom, r.astype(np.float64) / a.astype(np.float64), 1.0)
    l0, m0, f0 = lane(A0, R0)
    l1, m1, f1 = lane(A1, R1)
    bal = np.where((f0 >= 1.0) | (f1 >= 1.0), 0, ((1.0 - np.abs(f0 - f1)) * 100.0).astype(np.int64))
    least, most = (l0 + l1) // 2, (m0 + m1) // 2
    return least, most, bal, weights[0] * least + weights[1] * most + weights[2] * bal


def _edge_lanes():
    """(A, q, p) with R = q + p: A in {0, 1, 2^53 - 1, 2^53, INT64_MAX} x R in {-1, 0, A, A + 1, a wrapped sum}"""
    out = []
    for A in (0, 1, (1 << 53) - 1, 1 << 53, I64_MAX):
        for q, p in ((-1, 0), (0, 0), (A, 0), (A - 3, 3), (A, 1), (I64_MAX, 7), (I64_MIN + 50, -100)):
            out.append((A, q, p))
    return out


def _cases():
    rng = np.random.default_rng(77)
    edges = _edge_lanes()
    good = (4000, 1000, 500)
    cases = [(e, good) for e in edges] + [(good, e) for e in edges] + [(a, b) for a in edges[::4] for b in edges[::5]]
    for _ in range(600):
        lanes = []
        for hi in (64000, 1 << 38):
            A = int(rng.integers(1, hi))
            q = int(rng.integers(0, A + 1))
            lanes.append((A, q, int(rng.integers(0, A - q + 2))))
        cases.append(tuple(lanes))
    for _ in range(200):                                         # anything at all
        cases.append(tuple((int(rng.integers(I64_MIN, I64_MAX)), int(rng.integers(I64_MIN, I64_MAX)), int(rng.integers(I64_MIN, I64_MAX))) for _ in range(2)))
    for _ in range(200):                                         # large lanes around 2^53
        cases.append(tuple((int((1 << 53) + rng.integers(-5, 5)), int(rng.integers(0, 1 << 53)), int(rng.integers(0, 1 << 20))) for _ in range(2)))
    return cases


def _scalar(case, w):
    (A0, q0, p0), (A1, q1, p1) = case
    R0, R1 = ssr.nv.wrap64(q0 + p0), ssr.nv.wrap64(q1 + p1)
    return (R0, R1) + ssr.parts(A0, R0, A1, R1) + (ssr.total_of(A0, R0, A1, R1, w),)


def test_numpy_table_equals_the_scalar_function():
    cases = _cases()
    for w in [(1, 0, 1), (3, 2, 1), (65536, 65536, 65536), (0, 0, 0)]:
        want = np.array([_scalar(c, w) for c in cases], dtype=object)
        col = lambda j, k: np.array([c[j][k] for c in cases], np.int64)
        with np.errstate(over="ignore"):
            R0, R1 = col(0, 1) + col(0, 2), col(1, 1) + col(1, 2)           # int64 wraps
        assert R0.tolist() == list(want[:, 0]) and R1.tolist() == list(want[:, 1])
        got = table(col(0, 0), R0, col(1, 0), R1, w)
        for j, name in enumerate(("least", "most", "balanced", "total")):
            assert got[j].tolist() == list(want[:, 2 + j]), (w, name)
        assert max(want[:, 5]) < 1 << 32 and min(want[:, 5]) >= 0


def test_header_alone_under_sanitizers_equals_the_scalar_function(tmp_path):
    """csrc/bs_seq_score.hpp compiled alone (a plain host compile: no HIP header) with tests/native/seq_score_main.cpp under ASan + UBSan"""
    exe = str(tmp_path / "seq_score")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "seq_score_main.cpp"), "-o", exe], check=True)
    cases = _cases()
    for w in [(1, 0, 1), (3, 2, 1), (65536, 65536, 65536)]:
        text = "".join(f"{a[0]} {a[1]} {a[2]} {b[0]} {b[1]} {b[2]} {w[0]} {w[1]} {w[2]}\n" for a, b in cases)
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        lines = res.stdout.strip().splitlines()
        assert len(lines) == len(cases)
        for line, c in zip(lines, cases):
            assert tuple(int(x) for x in line.split()) == _scalar(c, w), (c, w, line)


# ---- the hand-computed answers -----------------------------------------------------------------------------------------------------------------
def test_hand_computed_nodes():
    kats = sss.load_kats()["nodes"]
    assert len(kats) >= 8
    for k in kats:
        R0, R1 = ssr.nv.wrap64(k["q0"] + k["p0"]), ssr.nv.wrap64(k["q1"] + k["p1"])
        assert ssr.parts(k["A0"], R0, k["A1"], R1) == (k["least"], k["most"], k["balanced"]), (k["name"], k["why"])
        assert ssr.total_of(k["A0"], R0, k["A1"], R1, (1, 0, 1)) == k["total_101"] == k["least"] + k["balanced"], k["name"]
        assert ssr.total_of(k["A0"], R0, k["A1"], R1, (3, 2, 1)) == k["total_321"] == 3 * k["least"] + 2 * k["most"] + k["balanced"], k["name"]
    assert {"quarter-full"} <= {k["name"] for k in kats}


def test_hand_derived_scenes():
    scenes = sss.load_kats()["scenes"]
    assert len(scenes) >= 2
    for k in scenes:
        sc = sss.kat_scene(k)
        assert {"1,0,1", "0,1,0", "0,0,0"} <= set(k["expect"])
        for wtext, nodes in k["expect"].items():
            w = tuple(int(x) for x in wtext.split(","))
            got = ssr.replay(sc, w)
            assert got["assumed"] == nodes == got["pod_node"], (k["name"], wtext, k["why"])
        assert ssr.replay(sc, (0, 0, 0))["pod_node"] == sor.replay(sc)["pod_node"]


# ---- the GPU scene set is not vacuous ---------------------------------------------------------------------------------------------------------------
# the scene of the committed lists (the parity set in order, each under the weights the GPU test runs it with, then the Filter family) that
# FIRST shows each hazard letter
FIRST = {"h": ("parity", 9100), "a": ("parity", 9101), "b": ("parity", 9101), "d": ("parity", 9101), "e": ("parity", 9101), "g": ("parity", 9101),
         "c": ("parity", 9102), "f": ("parity", 9103), "i": ("filter", 9105)}


def test_every_hazard_letter_on_its_first_scene():
    first, seen = {}, {c: 0 for c in ssr.HAZARDS}
    for i, (seed, n, S, gangs) in enumerate(sss.PARITY):
        sc = sss.parity_scene(seed, n, S, gangs)
        hz = ssr.replay(sc, sss.WEIGHTS[i % len(sss.WEIGHTS)], scalar_names=sc["names"])["hazards"]
        assert hz["i"] == 0, "no Filter, nothing removed"
        for c, v in hz.items():
            seen[c] += v
            if v:
                first.setdefault(c, ("parity", seed))
    for seed in sss.FILTER_SEEDS:
        sc = sss.filter_scene(seed)
        for deny in (False, True):
            hz = ssr.replay(sc, (1, 0, 1), run_filter=True, filter_deny=deny, scalar_names=sc["names"])["hazards"]
            seen["i"] += hz["i"]
            if hz["i"]:
                first.setdefault("i", ("filter", seed))
    assert first == FIRST, first
    assert all(seen[c] >= 1 for c in ssr.HAZARDS), seen
    assert seen["a"] >= 100 and seen["b"] >= 50 and seen["f"] >= 50 and seen["d"] >= 50, seen


def test_built_scenes_do_what_their_names_say():
    spread, pack = ssr.replay(sss.identical(), (1, 0, 1)), ssr.replay(sss.identical(), (0, 1, 0))
    assert spread["assumed"] == [i % 8 for i in range(20)], "least requested + balanced spreads"
    assert pack["assumed"] == [i // 8 for i in range(20)] and pack["hazards"]["g"] == 2, "most requested packs, eight pods fill a node to the brim"
    wild = ssr.replay(sss.out_of_domain(), (1, 0, 1))
    assert wild["hazards"]["d"] == 18 and {0, 2, 5} <= set(wild["assumed"]), "nodes with a lane out of domain are candidates and are chosen"
    waves = ssr.replay(sss.geometry_waves(), (1, 0, 1))
    assert waves["assumed"][:4] == [65 * 64 + 5, 66 * 64 + 1, 66 * 64 + 9, 64 * 64 + 5], waves["assumed"]
    assert all(n == 5 for n in waves["n_fit"]) and waves["hazards"]["f"] == 6


# ---- where the new kernels sit -----------------------------------------------------------------------------------------------------------------
def test_thirteen_scored_instantiations_without_scratch_in_a_unit_of_their_own():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources(bsa.build.build())
    scored = {k: v for k, v in all_k.items() if "k_seq_scored" in k}
    passes = {k: v for k, v in all_k.items() if "k_seq_pass" in k}
    assert len(scored) == 13 and len(passes) == 12, (sorted(scored), sorted(passes))       # (0 .. 12 scalar lanes, no generic-lane one: see bs_seq.hpp)
    assert all(v["scratch"] == 0 for v in scored.values()), scored
    units = {v["unit"] for v in scored.values()}
    assert len(units) == 1 and units.isdisjoint({v["unit"] for k, v in all_k.items() if k not in scored}), "nothing but the thirteen kernels in tu_seq_score.hip"
    assert "tu_seq_score.hip" in bsa.build.SOURCES
    summary = open(os.path.join(ROOT, "profiles", "seq_scored_isa_diff.txt")).read()
    for k in passes:
        assert any(line.startswith("same " + k + " ") for line in summary.splitlines()), k
