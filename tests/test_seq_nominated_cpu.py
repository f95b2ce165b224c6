"""CPU tests of bs_seq_run_nominated's rule (include/bsched.h, rule S and D6): the object-level model tests/seq_nominated_ref.py pinned
against the two existing statements of the sequential pass, the hand-derived answers (tests/golden/seq_nominated_hand_kats.json), the
non-vacuity of the random scene set the GPU tests run, the host-side own-id check alone under the sanitizers, and where the new kernels sit
in the build.  No GPU: nothing here creates a context."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import naive_ref as nv
import seq_nominated_ref as snr
import seq_nominated_scenes as sns
import seq_obj_replay as sor
from test_seq_oracle_pin import _assert_same, _c_pass, _with_waiting

bsa = importlib.import_module("batch-scheduler_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M64 = (1 << 64) - 1


def _scene(seed):
    if seed % 3 == 0:
        return _with_waiting(seed)
    if seed % 3 == 1:
        return _with_waiting(seed, n_nodes=int(6 + seed % 7), n_groups=int(2 + seed % 4), n_pods=int(20 + seed % 17), edge=False)
    return _with_waiting(seed, n_nodes=int(3 + seed % 5), n_groups=3, n_pods=30, n_scalars=seed % 3, edge=True)


# ---- pin 1: with no rows the model is the sequential pass ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(120))
def test_without_rows_the_model_is_the_object_replay_and_the_c_pass(orc, soa, seed):
    sc, closed = _scene(seed)
    prio = np.random.default_rng(seed).integers(-3, 40, size=len(sc["pods"]))
    got = snr.replay(sc, [], prio, None, closed, scalar_names=sc["names"])
    obj = sor.replay(sc, closed, scalar_names=sc["names"])
    for k in ("pf_code", "pf_first_k", "pf_leader", "pod_node", "released_group", "released_pods", "matched", "status_scheduled", "latch", "closed", "denied"):
        assert got[k] == obj[k], (seed, k)
    assert got["consumed"] == [] and got["nominees"] == [] and got["blocked"] == 0
    c, _ = _c_pass(orc, soa, sc, closed, soa.STAGE_PREFILTER)
    _assert_same(soa, got, c, f"seed {seed}")
    owner_ids = {}
    nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], sc["names"], sc["n_classes"], sc["denied"], sc["permitted"], owner_ids=owner_ids)
    nodes, groups, _ = snr.end_state_soa(got, sc, soa, owner_ids)
    assert np.array_equal(nodes.requested, c["nodes"].requested) and np.array_equal(nodes.requested_present, c["nodes"].requested_present), seed
    assert np.array_equal(groups.flags, c["groups"].flags) and np.array_equal(groups.matched, c["groups"].matched), (seed, groups.flags, c["groups"].flags)
    assert np.array_equal(groups.occupied_by, c["groups"].occupied_by), seed


# ---- pin 2: one priority, no own rows: the C pass on nodes that carry the rows' sums ---------------------------------------------------------
def _pin2_scene(seed):
    """ungrouped pods only (PreFilter reads the plugin's own NodeInfo, rule S1: with groups the C pass on inflated nodes would scan other sums
    than the model's), one or two scalars, rows on random nodes with priorities around P"""
    rng = np.random.default_rng(seed)
    S = 1 + seed % 2
    sc = sns.scenarios.random_objects(seed, n_nodes=int(4 + seed % 9), n_groups=2, n_pods=int(20 + seed % 13), n_scalars=S, n_classes=2, edge=(seed % 4 == 0))
    for pod in sc["pods"]:
        pod.group = None
    sc["permitted"] = set()
    P = 10
    rows = []
    for r in range(int(rng.integers(1, 3 * len(sc["nodes"])))):
        rq = {"cpu": int(rng.choice([0, 500, 4000, 20000])), "memory": int(rng.choice([0, 1, 8])) * sns.GI}
        for nm in sc["names"]:
            if rng.random() < 0.5:
                rq[nm] = int(rng.choice([0, 1, 4, 8]))
        rows.append(snr.Nominee(r, int(rng.integers(0, len(sc["nodes"]))), P + int(rng.integers(-2, 3)), sns._row_req(rq, sc["names"])))
    return sc, P, rows


@pytest.mark.parametrize("seed", range(2000, 2110))
def test_one_priority_the_model_is_the_c_pass_on_nodes_that_carry_the_sums(orc, soa, seed):
    sc, P, rows = _pin2_scene(seed)
    names, L = sc["names"], 4 + len(sc["names"])
    got = snr.replay(sc, rows, [P] * len(sc["pods"]), None, scalar_names=names)
    nodes, fit, groups, pods, _ = nv.to_soa(sc["nodes"], sc["cache"], sc["pods"], names, sc["n_classes"], sc["denied"], sc["permitted"])
    cols = snr.objects_to_rows([o for o in rows if o.priority >= P], names)
    add, bits = np.zeros((L, nodes.n), object), np.zeros(nodes.n, np.uint32)
    add[:] = 0
    for i in range(len(cols["id"])):
        k = int(cols["node"][i])
        for j in range(L):
            add[j, k] += int(cols["req"][j, i])
        bits[k] |= cols["req_present"][i]
    heavy = nodes.copy()
    for k in range(nodes.n):
        for j in range(L):
            present = j < 4 or (int(nodes.requested_present[k]) >> (j - 4)) & 1           # AddPod: an absent key counts as 0
            heavy.requested[j, k] = np.int64(snr.nv.wrap64((int(nodes.requested[j, k]) if present else 0) + int(add[j, k])))
    heavy.requested_present |= bits
    c = orc.seq_replay(heavy, fit, groups, pods, soa.STAGE_PREFILTER)
    assert list(c["pod_node"]) == got["pod_node"] == got["assumed"], seed
    end, _, _ = snr.end_state_soa(got, sc, soa, {})
    for k in range(nodes.n):
        for j in range(L):
            assert snr.nv.wrap64(int(c["nodes"].requested[j, k]) - int(add[j, k])) == int(end.requested[j, k]), (seed, j, k)
    assert np.array_equal(c["nodes"].requested_present, end.requested_present | bits), seed


def test_the_pin2_scenes_use_scalars_and_rows_decide():
    scal = moved = 0
    for seed in range(2000, 2110):
        sc, P, rows = _pin2_scene(seed)
        got = snr.replay(sc, rows, [P] * len(sc["pods"]), None, scalar_names=sc["names"])
        scal += int(any(o.req.ScalarResources for o in rows))
        moved += int(got["blocked"] > 0)
    assert scal >= 100 and moved >= 40, (scal, moved)


# ---- hand-derived answers ------------------------------------------------------------------------------------------------------------------
KATS = sns.load_kats()


def test_the_golden_file_has_one_scene_per_hazard():
    assert [k["name"] for k in KATS] == list("abcdefghijklm")
    for k in KATS:
        if k["name"] in "efklm":                                # the cursor scenes span two tiles of 64 nodes
            assert len(sns.kat_scene(k)["sc"]["nodes"]) >= 65 and min(k["expect_node"]) < 64 <= max(k["expect_node"])


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_hand_answers(kat):
    scn = sns.kat_scene(kat)
    got = snr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], scalar_names=scn["names"])
    assert got["assumed"] == kat["expect_node"], kat["why"]
    assert [o.id for o in got["nominees"]] == kat["expect_rows"], kat["why"]
    assert got["hazards"][kat.get("hazard", kat["name"])] >= 1, f"scene {kat['name']} does not reach its hazard: {got['hazards']}"
    if kat["name"] == "g":
        assert got["pf_code"][0] >= 16
    if kat["name"] == "h":
        assert got["pod_node"][0] == -1 and got["consumed"] == [(0, 0, 0)]
    if kat["name"] == "i":
        assert not (got["op"].nodes[0].requested.ScalarResources or {})


# ---- the random scene set of the GPU tests is not vacuous -----------------------------------------------------------------------------------
def test_the_gpu_scene_set_differs_from_the_rowless_pass_and_meets_every_hazard():
    differ, hz = 0, {c: 0 for c in snr.HAZARDS}
    for seed, n, m in sns.PARITY:
        scn = sns.parity_scene(seed, n, m)
        got = snr.replay(scn["sc"], scn["nominees"], scn["priority"], scn["own_id"], scalar_names=scn["names"])
        differ += int(got["pod_node"] != scn["rowless"]["pod_node"])
        for c, v in got["hazards"].items():
            hz[c] += v
    assert len(sns.PARITY) >= 40 and {n for _, n, _ in sns.PARITY} == {48, 130, 200} and {m for _, _, m in sns.PARITY} == {1, 7, 64, 300}
    assert 2 * differ >= len(sns.PARITY), (differ, len(sns.PARITY))
    # a-j: the issue's list; e, f and k are counted at the granularity of the kernel's cursors (another TILE of 64 nodes, or a hit after a
    # search that found nothing), so the cursors-on and cursors-off runs of the GPU tests really walk different paths there.  l (a row that
    # grows the room) does not come up at random: the hand scenes l and m put it across two tiles.
    assert all(hz[c] >= 1 for c in "abcdefghijk"), hz
    assert hz["e"] >= 5 and hz["f"] >= 5 and hz["k"] >= 2, hz


# ---- the own-id check alone, under the sanitizers -----------------------------------------------------------------------------------------------
def test_own_id_check_under_sanitizers(tmp_path):
    """csrc/bs_nominated_check.hpp's nom_own_check compiled alone with tests/native/seq_nominated_check_main.cpp under ASan + UBSan: every
    refusal, the translation to row indices, arrays of exactly the stated sizes"""
    exe = str(tmp_path / "own_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "seq_nominated_check_main.cpp"), "-o", exe], check=True)
    none = 0xFFFFFFFF
    cases = [  # (live, ids, own or None) -> (code, rows)
        (([], 0, None, 3), (0, [none] * 3)),
        (([], 0, [none, none], 2), (0, [none, none])),
        (([2, 5, 9], 10, [9, none, 2, none], 4), (0, [2, none, 0, none])),
        (([2, 5, 9], 10, [10], 1), (3, None)),                   # unknown: at the id space
        (([2, 5, 9], 10, [4], 1), (4, None)),                    # dead
        (([], 10, [4], 1), (4, None)),                           # dead: empty table
        (([2, 5, 9], 10, [5, none, 5], 3), (5, None)),           # named by two pods
        (([0], 1, [0], 1), (0, [0])),
        (([7], 8, [], 0), (0, [])),
    ]
    text = ""
    for (live, ids, own, p), _ in cases:
        text += f"{len(live)} {' '.join(map(str, live))} {ids} {p} {0 if own is None else 1} {' '.join(map(str, own or []))}\n"
    res = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for line, (_, (code, rows)) in zip(lines, cases):
        f = [int(x) for x in line.split()]
        assert f[0] == code, line
        if code == 0:
            assert f[1:] == rows, line


# ---- where the new kernels sit -----------------------------------------------------------------------------------------------------------------
# Scratch of k_seq_pass<TS, true> beyond its flag-less sibling's (bytes).  The NOM instantiation carries one more int64 per resource lane
# through the tile test (the rows' sum beside the raw requests the assume step writes from).  With 0..2 scalar lanes that fits the register
# file; k_seq_pass<3> and <4> already sit at 241 and 256 of 256 VGPRs and the generic-lane instantiation spills before the change, so those
# three spill the difference.  The pass is one persistent launch: the set-up is paid once per pass.
EXTRA_SCRATCH = {"0": 0, "1": 0, "2": 0, "3": 16, "4": 64, "n1": 160}            # measured: 12, 60 and 148 bytes


def test_six_nominated_instantiations_their_scratch_and_their_unit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources(bsa.build.build())
    plain = {k: v for k, v in all_k.items() if "k_seq_pass" in k and "Lb1" not in k}
    nom = {k: v for k, v in all_k.items() if "k_seq_pass" in k and "Lb1" in k}
    assert len(plain) == 6 and len(nom) == 6, (sorted(plain), sorted(nom))
    for k, v in nom.items():
        ts = k.split("k_seq_passIL")[1].split("ELb1")[0][1:]            # "i0" .. "i4", "in1" -> "0" .. "4", "n1"
        sib = [p for p in plain if f"k_seq_passILi{ts}EE" in p]
        assert len(sib) == 1, (k, sib)
        assert v["scratch"] <= plain[sib[0]]["scratch"] + EXTRA_SCRATCH[ts], (k, v["scratch"], plain[sib[0]]["scratch"])
    units = {v["unit"] for v in nom.values()}
    assert len(units) == 1
    assert units.isdisjoint({v["unit"] for k, v in all_k.items() if "k_nm_" in k or "k_wt_" in k or "k_se_" in k})
    assert units.isdisjoint({v["unit"] for v in plain.values()}), "the flag-less instantiations keep a unit of their own (profiles/seq_nominated_isa_diff.txt)"
