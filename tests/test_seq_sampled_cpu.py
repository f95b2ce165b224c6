"""CPU tests of rule F (include/bsched.h: bs_seq_run_scored_sampled, bs_seq_run_scored_nominated_sampled; D9, F1, F2): the object-level
model tests/seq_sampled_ref.py against its second statement from arrays (tests/seq_sampled_soa.py) on seeded scenes and on the scenes the GPU
tests run; F1 against the parent models on every scene; F2 against a rotated first fit; D9 on upstream's table; csrc/bs_seq_sample.hpp compiled
alone under the sanitizers; the hand-derived answers (tests/golden/seq_sampled_hand_kats.json); the census of hazards over the very cases the GPU
tests run; and where the new kernels sit in the build.  No GPU: nothing here creates a context."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import seq_nominated_ref as snr
import seq_sampled_ref as smr
import seq_sampled_scenes as sms
import seq_sampled_soa as smsoa
import seq_scored_nominated_ref as spr
import seq_scored_nominated_scenes as sps
import seq_scored_ref as ssr
import seq_scored_scenes as sss
import seq_soa_ref as ssoa
from test_gpu_seq import assert_groups_equal

bsa = importlib.import_module("batch-scheduler_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEQ = ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods")
END = ("matched", "status_scheduled", "latch", "closed", "denied")
KATS = sms.load_kats()

# the seeded scenes the two models are held together on: (seed, nodes, scalar lanes, gangs, form)
SEEDED = [(9700 + i, (48, 65, 130, 70)[i % 4], i % 3, i % 5 != 4, "SP" if i % 3 == 2 else "P") for i in range(210)]


def _seeded(seed, n, S, gangs, form):
    if form == "P":
        sc = sss.make(seed, n_nodes=n, n_groups=6, n_pods=30, n_scalars=S, gangs=gangs)
        return dict(sc=sc, names=sc["names"], nominees=None, priority=None, own_id=None)
    return sps.make(seed, n, (7, 64, 1)[seed % 3], S, weights=(1, 0, 1), n_pods=30)


def _sample_of(seed, n):
    """a sample that lets the walk stop, wrap, or see everything, by the seed"""
    return ((1, 2, 5, 17, 64, 0, n, n + 1)[seed % 8], (0, 1, 63, 64, n - 1, n, n + 7, 31)[(seed // 8) % 8])


def _soa(scn):
    if scn["nominees"] is None:
        return sss.to_soa(scn["sc"]) + (None,)
    return sps.to_soa(scn)


def _array_model(orc, scn, weights, sample):
    """the array model's pass over a scene -> (seq_pass's dict, the choice object)"""
    nodes, fit, groups, pods, owner_ids, rows = _soa(scn)
    nom = None if scn["nominees"] is None else ssoa.NominatedChoice(rows, scn["priority"], scn["own_id"])
    ch = smsoa.SampledChoice(sample, weights, pods.p, nodes.n, nom)
    return ssoa.seq_pass(orc, nodes, fit, groups, pods, -1, ch), ch, owner_ids


def _object_model(scn, weights, sample):
    return smr.replay(scn["sc"], weights, sample, scalar_names=scn["names"], nominees=scn["nominees"], priority=scn["priority"], own_id=scn["own_id"])


def _models_agree(orc, soa, scn, weights, sample, where):
    model = _object_model(scn, weights, sample)
    got, ch, owner_ids = _array_model(orc, scn, weights, sample)
    for k in SEQ + ("assumed",):
        assert got[k].tolist() == list(model[k]), f"{where}: {k}"
    assert ch.total.tolist() == model["total"] and ch.n_fit.tolist() == model["n_fit"], f"{where}: totals and kept counts"
    assert ch.start.tolist() == model["start"] and ch.visited.tolist() == model["visited"] and ch.next_start == model["next_start"], f"{where}: the cursor"
    en, eg, wait = smr.end_state_soa(model, scn["sc"], soa, dict(owner_ids))
    assert np.array_equal(got["nodes"].requested, en.requested) and np.array_equal(got["nodes"].requested_present, en.requested_present), f"{where}: node requests"
    assert_groups_equal(got["groups"], eg, soa, where)
    assert np.array_equal(got["wait_node"], wait), f"{where}: the pods that wait at Permit"
    if scn["nominees"] is not None:
        assert sorted(ch.consumed) == model["consumed"], f"{where}: consumed rows"
        assert ch.live_ids().tolist() == [o.id for o in model["nominees"]], f"{where}: surviving rows"
    return model


# ---- the two statements of rule F ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,S,gangs,form", SEEDED, ids=[f"{s}-N{n}-S{S}-{'gangs' if g else 'single'}-{f}" for s, n, S, g, f in SEEDED])
def test_the_object_model_is_the_array_model(seed, n, S, gangs, form, orc, soa):
    scn = _seeded(seed, n, S, gangs, form)
    weights = (0, 0, 0) if seed % 7 == 6 else sss.WEIGHTS[seed % len(sss.WEIGHTS)]
    model = _models_agree(orc, soa, scn, weights, _sample_of(seed, n), f"seed {seed}")
    assert len(SEEDED) >= 200 and sum(1 for a in model["assumed"] if a >= 0) > 0


CROSS = sms.LANE_CASES[:3] + sms.LANE_CASES[6:9] + sms.KNOWN_CASES + [sms.PRUNE_CASE] + sms.GRID_SP[::7] + sms.GRID_P[::29]


@pytest.mark.parametrize("case", CROSS, ids=["-".join(str(x) for x in c) for c in CROSS])
def test_the_two_models_agree_on_cases_the_gpu_tests_run(case, orc, soa):
    key, sample, weights, flt = sms.split(case)
    assert not flt, "the array model is PreFilter-only"
    _models_agree(orc, soa, sms.scene(case), weights, sample, str(case))


# ---- F1: K = all, start = 0 is the parent form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n,S,gangs,form", SEEDED, ids=[f"{s}-N{n}-S{S}-{'gangs' if g else 'single'}-{f}" for s, n, S, g, f in SEEDED])
def test_f1_all_nodes_from_cursor_zero_is_the_parent_model(seed, n, S, gangs, form):
    scn = _seeded(seed, n, S, gangs, form)
    w = sss.WEIGHTS[seed % len(sss.WEIGHTS)]
    a = _object_model(scn, w, ((0, n, n + 1)[seed % 3], (0, n)[seed % 2]))
    if form == "P":
        b = ssr.replay(scn["sc"], w, scalar_names=scn["names"])
    else:
        b = spr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], w, scalar_names=scn["names"])
        assert a["consumed"] == b["consumed"] and [o.id for o in a["nominees"]] == [o.id for o in b["nominees"]], seed
    for k in SEQ + END + ("assumed", "total", "n_fit", "last_permitted"):
        assert a[k] == b[k], (seed, k)
    reached = [i for i in range(len(a["start"])) if a["n_fit"][i] or a["visited"][i]]
    assert all(a["start"][i] == 0 for i in range(len(a["start"]))) and all(a["visited"][i] == n for i in reached) and a["next_start"] == 0
    assert not any(a["hazards"][c] for c in "abcdefghijkl"), a["hazards"]
    for info_a, info_b in zip(a["op"].nodes, b["op"].nodes):
        assert info_a.requested == info_b.requested and info_a.pod_count == info_b.pod_count


@pytest.mark.parametrize("seed", sss.FILTER_SEEDS)
def test_f1_with_the_filter_stage(seed):
    sc = sss.filter_scene(seed)
    a = smr.replay(sc, (1, 0, 1), (0, 0), run_filter=True, scalar_names=sc["names"])
    b = ssr.replay(sc, (1, 0, 1), run_filter=True, scalar_names=sc["names"])
    for k in SEQ + END + ("assumed", "total", "n_fit"):
        assert a[k] == b[k], (seed, k)


# ---- F2: zero weights are first fit from a rotating start ----------------------------------------------------------------------------------------
def _rotated_first_fit(orc, scn, sample):
    """seq_soa_ref.seq_pass with a choice that knows nothing of totals: the first member of C at or behind the cursor, else C's first; the
    cursor then moves by the distance to the NEXT member (K = 1: the walk ends on the second member) or stays (one member or none)"""
    nodes, fit, groups, pods, _, _ = _soa(scn)
    N = nodes.n
    state = dict(s=sample[1] % N)

    def choose(i, C, work):
        s = state["s"]
        behind = [k for k in C if k >= s] + [k for k in C if k < s]
        if len(behind) > 1:
            state["s"] = behind[1]
        return behind[0] if behind else -1
    return ssoa.seq_pass(orc, nodes, fit, groups, pods, -1, choose), state["s"]


@pytest.mark.parametrize("seed,n,S,gangs,form", [c for c in SEEDED if c[4] == "P"][:40], ids=str)
def test_f2_zero_weights_are_a_rotated_first_fit(seed, n, S, gangs, form, orc):
    scn = _seeded(seed, n, S, gangs, form)
    start = _sample_of(seed, n)[1]
    model = _object_model(scn, (0, 0, 0), (1, start))
    got, cursor = _rotated_first_fit(orc, scn, (1, start))
    for k in SEQ + ("assumed",):
        assert got[k].tolist() == list(model[k]), (seed, k)
    assert cursor == model["next_start"] and not any(model["total"])
    # ... and with any K the zero-weight choice is still the first member in visit order: the same nodes as long as the walks start alike
    wide = _object_model(scn, (0, 0, 0), (5, start))
    first = next((i for i, a in enumerate(model["assumed"]) if a >= 0), None)
    assert first is None or wide["assumed"][first] == model["assumed"][first]


# ---- D9 -------------------------------------------------------------------------------------------------------------------------------------------
D9_UPSTREAM = [(0, 10, 10), (40, 10, 10), (0, 1000, 420), (40, 1000, 400), (0, 6000, 300), (40, 6000, 2400), (0, 5000, 500)]
# n = 99, 100, 125, 5 000, 20 000 under percentage = -1, 0, 5, 99, 100, worked out from the rule by hand
D9_HAND = {99: {-1: 99, 0: 99, 5: 99, 99: 99, 100: 99},                          # below 100 nodes: all
           100: {-1: 100, 0: 100, 5: 100, 99: 100, 100: 100},                    # 50 - 0 = 50 % of 100 = 50, 5 and 99 likewise: all raised to 100
           125: {-1: 100, 0: 100, 5: 100, 99: 123, 100: 125},                    # 49 % = 61 -> 100; 5 % = 6 -> 100; 99 % = 123.75 -> 123
           5000: {-1: 500, 0: 500, 5: 250, 99: 4950, 100: 5000},                 # 50 - 40 = 10 %
           20000: {-1: 1000, 0: 1000, 5: 1000, 99: 19800, 100: 20000}}           # 50 - 160 -> 5 %


def test_d9_on_upstreams_table_and_the_edges():
    lib = bsa.capi.load_library()
    for pct, n, want in D9_UPSTREAM:
        assert smr.sample_size(n, pct) == want == bsa.capi.seq_sample_size(n, pct) == lib.bs_seq_sample_size(n, pct), (pct, n)
    for n, row in D9_HAND.items():
        for pct, want in row.items():
            assert smr.sample_size(n, pct) == want == bsa.capi.seq_sample_size(n, pct), (n, pct)
    assert bsa.capi.seq_sample_size(5000) == 500 and bsa.capi.seq_sample_size(20000) == 1000


def test_header_alone_under_sanitizers(tmp_path):
    """csrc/bs_seq_sample.hpp compiled alone (a plain host compile: no HIP header) with tests/native/seq_sample_main.cpp under ASan + UBSan:
    its own checks, then the D9 vectors, the rotation at s = 0, 1, 63, 64, N - 1 and the r-th set bit on the masks the issue names"""
    exe = str(tmp_path / "seq_sample")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "seq_sample_main.cpp"), "-o", exe], check=True)
    lines, want = [], []
    for pct, n, w in D9_UPSTREAM:
        lines.append(f"size {n} {pct}")
        want.append(str(w))
    for n, row in D9_HAND.items():
        for pct, w in row.items():
            lines.append(f"size {n} {pct}")
            want.append(str(w))
    for N in (1, 64, 65, 513):
        for s in (0, 1, 63, 64, N - 1):
            s0 = s % N
            k1 = (s0 + (1 if N > 1 else 0)) % N
            lines.append(f"walk {s} {N}")
            want.append(f"{s0} {k1} {(s0 + N - 1) % N} {(k1 - s0) % N} {s0}")
    ones, even, odd = (1 << 64) - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA
    for mask, r, w in [(ones, 1, 0), (ones, 64, 63), (ones, 65, 64), (1 << 63, 1, 63), (1, 1, 0), (1 << 31, 1, 31), (1 << 32, 1, 32), (even, 1, 0), (even, 32, 62),
                       (odd, 1, 1), (odd, 32, 63), (odd, 33, 64), (0, 1, 64), (ones, 0, 64)]:
        lines.append(f"bit {mask:x} {r}")
        want.append(str(w))
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    out = res.stdout.strip().splitlines()
    assert out[0] == "self-check ok" and out[1:] == want, [(a, b) for a, b in zip(out[1:], want) if a != b]


# ---- the hand-derived answers -----------------------------------------------------------------------------------------------------------------
def test_the_golden_file_has_at_least_twelve_scenes_of_both_forms():
    assert len(KATS) >= 12 and {k["form"] for k in KATS} == {"P", "SP"}
    assert len({k["name"] for k in KATS}) == len(KATS) and all(k["why"] for k in KATS)


@pytest.mark.parametrize("i", range(len(KATS)), ids=[k["name"] for k in KATS])
def test_hand_answers_both_models(i, orc, soa):
    kat, case = KATS[i], ("kat", KATS[i]["form"], i)
    model = _models_agree(orc, soa, sms.scene(case), tuple(kat["weights"]), tuple(kat["sample"]), kat["name"])
    ex = kat["expect"]
    for k in ("start", "visited", "n_fit", "total", "assumed", "next_start"):
        assert model[k] == ex[k], (kat["name"], k, kat["why"])
    if kat["form"] == "SP":
        assert [o.id for o in model["nominees"]] == ex["rows_left"], (kat["name"], kat["why"])


# ---- the census of the cases the GPU tests run --------------------------------------------------------------------------------------------------
def test_the_gpu_cases_meet_every_hazard():
    cases = sms.all_gpu_cases()
    assert len(set(cases)) == len(cases)
    seen = {c: 0 for c in smr.HAZARDS + smr.EXTRA}
    by_form = {"P": dict(seen), "SP": dict(seen)}
    placed = 0
    for case in cases:
        md = sms.model(case)
        for c in seen:
            seen[c] += md["hazards"][c]
            by_form[case[1]][c] += md["hazards"][c]
        placed += sum(1 for a in md["assumed"] if a >= 0)
    assert all(seen[c] >= 1 for c in smr.HAZARDS + smr.EXTRA), seen
    assert all(by_form["P"][c] >= 1 for c in "abcdefghij") and all(by_form["SP"][c] >= 1 for c in "abcegijkl"), by_form
    assert by_form["P"]["k"] == by_form["P"]["l"] == 0, "rows exist under rule SP only"
    assert placed >= 5000, placed
    # the grid is the issue's: every N with every distinct cursor and every sample size
    grid = {(c[2], c[3], c[4]) for c in sms.GRID_P}
    assert grid == {(ni, s, k) for ni, n in enumerate(sms.GRID_N) for s in sms.starts(n) for k in sms.sizes(n)}
    assert sms.GRID_N == [1, 63, 64, 65, 128, 129, 511, 512, 513, 1025]
    for ni, n in enumerate(sms.GRID_N):
        sp = [c for c in sms.GRID_SP if c[2] == ni]
        assert {c[3] for c in sp} == set(sms.starts(n)) and {c[4] for c in sp} == set(sms.sizes(n)), n


def test_built_scenes_do_what_their_names_say():
    pr = sms.model(sms.PRUNE_CASE)
    assert (pr["start"][0], pr["visited"][0], pr["n_fit"][0]) == (200, 130 + sms.PRUNE_N - 200, 5), "the walk from 200 ends on node 130, across excluded tile 1"
    assert pr["assumed"][0] in (260, 330, 390, 3, 10) and pr["start"][1] == 130
    for case, (fit, v) in zip(sms.KNOWN_CASES, [(11, None), (12, 200), (12, 200)]):
        md = sms.model(case)
        assert md["n_fit"] == [fit] * 10 and (v is None or md["visited"] == [v] * 10), case
    assert all(x < 200 for x in sms.model(sms.KNOWN_CASES[0])["visited"]), "K = |C| - 1 stops every walk"
    assert sms.model(sms.KNOWN_CASES[1])["hazards"]["h"] == 10 and sms.model(sms.KNOWN_CASES[2])["hazards"]["i"] == 10
    far = {c[3]: sms.model(c) for c in sms.FAR_CASES}
    assert far[1]["visited"][0] == 512 and far[1]["hazards"]["x"] >= 1 and far[1]["hazards"]["d"] >= 1, "K = 1: the second member opens round 1"
    assert far[2]["visited"][0] == 522 and far[4]["visited"][0] == 1016 and far[5]["visited"][0] == 1019
    assert far[5]["hazards"]["f"] >= 1, "K = 5: the sixth member sits in the revisited low lanes of the cursor's tile"
    fl = sms.model(sms.FILTER_CASE)
    assert fl["hazards"]["m"] >= 1, "Filter removes the node that would have been the K-th member"


# ---- where the new kernels sit -----------------------------------------------------------------------------------------------------------------
def test_two_families_of_thirteen_without_scratch_each_in_a_unit_of_its_own():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources(bsa.build.build())
    nom = {k: v for k, v in all_k.items() if "k_seq_sampled_nom" in k}
    plain = {k: v for k, v in all_k.items() if "k_seq_sampled" in k and k not in nom}
    assert len(plain) == 13 and len(nom) == 13, (sorted(plain), sorted(nom))      # 0 .. 12 scalar lanes each, no generic-lane one (bs_seq.hpp)
    for fam in (plain, nom):
        assert all(v["scratch"] == 0 and v["vgpr"] <= 256 for v in fam.values()), fam   # 512 threads on one CU: two waves per SIMD, 256 VGPRs
        assert all(v["lds"] <= 64 * 1024 for v in fam.values()), "the static part leaves the dynamic window its room"
        units = {v["unit"] for v in fam.values()}
        assert len(units) == 1 and units.isdisjoint({v["unit"] for k, v in all_k.items() if k not in fam}), "nothing but the thirteen kernels in the unit"
    assert not any(s in k for k in list(plain) + list(nom) for s in ("k_seq_pass", "k_seq_scored", "k_seq_sp")), "the other families are counted by name"
    assert "tu_seq_sample.hip" in bsa.build.SOURCES and "tu_seq_sample_nom.hip" in bsa.build.SOURCES
    assert "bs_seq_sample.hpp" in bsa.build.UNITS["tu_seq_sample.hip"] and "bs_seq_sample.hpp" in bsa.build.UNITS["tu_seq.hip"]
    summary = open(os.path.join(ROOT, "profiles", "seq_sampled_isa_diff.txt")).read()
    old = [k for k in all_k if "k_seq_pass" in k or "k_seq_scored" in k or "k_seq_sp" in k]
    assert len(old) == 12 + 13 + 13
    for k in old:
        assert any(line.startswith("same " + k + " ") for line in summary.splitlines()), k
