"""CPU checks of the resident PodDisruptionBudgets: the by-id model of tests/pdb_resident_ref.py, fed by pdb.matching_members and
pdb.allowed_vector, equals pdb.violating_bits (the path it replaces) on seeded scenes of string records, before and after budgets are
flipped; the model gives the hand known answers of tests/golden/pdb_resident_hand_kats.json; the header declares the four calls with the
argument lists the binding gives them, and the ABI version is still 7."""
import ctypes
import importlib
import os
import re

import numpy as np

import pdb_resident_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bsa = importlib.import_module("batch-scheduler_amd")
pdb, capi = bsa.pdb, bsa.capi


def _parses(sel):
    try:
        return pdb.parse_selector(sel)
    except ValueError:
        return "broken"


def test_model_equals_violating_bits_on_string_scenes():
    seen = dict(broken=0, nil=0, empty=0, bare=0, ops=set(), budgets=set(), namespaces=set(), set_bits=0, clear_bits=0, flipped=0)
    for seed in range(320):
        pdbs, pods = pr.string_scene(seed)
        for p in pdbs:
            r = _parses(p["selector"])
            seen["broken"] += r == "broken"
            seen["nil"] += r is None
            seen["empty"] += r == []
            if isinstance(r, list):
                seen["ops"] |= {op for _, op, _ in r}
            seen["budgets"].add(p["disruptions_allowed"])
            seen["namespaces"].add(p["namespace"])
        seen["bare"] += sum(1 for q in pods if not q["labels"])
        off, member = pdb.matching_members(pdbs, pods)
        allowed = pdb.allowed_vector(pdbs)
        assert off.dtype == np.uint32 and member.dtype == np.uint32 and allowed.dtype == np.int32
        assert off.size == len(pods) + 1 and off[0] == 0 and off[-1] == member.size and np.all(np.diff(off.astype(np.int64)) >= 0)
        assert allowed.size == len(pdbs) and (member.size == 0 or member.max() < len(pdbs))
        m = pr.Model(allowed, off, member)
        want = pdb.violating_bits(pdbs, pods)
        assert np.array_equal(m.bits(len(pods)), want), f"seed {seed}"
        seen["set_bits"] += int(want.sum())
        seen["clear_bits"] += int((want == 0).sum())
        # budgets flip; the memberships do not move (disruptions_allowed is no input of matching_members)
        rng = np.random.default_rng(seed + 5000)
        for _ in range(3):
            if not pdbs:
                break
            idx = rng.permutation(len(pdbs))[: int(rng.integers(1, len(pdbs) + 1))]
            val = rng.choice(np.array(pr.BUDGETS, np.int64), idx.size)
            for i, v in zip(idx, val):
                pdbs[int(i)]["disruptions_allowed"] = int(v)
            m.allowed_apply(idx, val)
            again = pdb.matching_members(pdbs, pods)
            assert np.array_equal(again[0], off) and np.array_equal(again[1], member)
            assert np.array_equal(m.allowed, pdb.allowed_vector(pdbs))
            after = pdb.violating_bits(pdbs, pods)
            assert np.array_equal(m.bits(len(pods)), after), f"seed {seed} after a flip"
            seen["flipped"] += int((after != want).any())
            want = after
    assert seen["broken"] > 20 and seen["nil"] > 10 and seen["empty"] > 10 and seen["bare"] > 100, seen
    assert seen["ops"] == {"In", "NotIn", "Exists", "DoesNotExist"} and seen["budgets"] >= {0, 1, -1, pr.I32_MIN, pr.I32_MAX}, seen
    assert seen["namespaces"] == set(pr.NAMESPACES) and seen["set_bits"] > 300 and seen["clear_bits"] > 300 and seen["flipped"] > 100, seen


def test_a_pdb_that_matches_nobody_keeps_its_index():
    pods = [{"namespace": "default", "labels": {"app": "a"}}, {"namespace": "other", "labels": {"app": "a"}}, {"namespace": "default", "labels": None}]
    good = {"matchLabels": {"app": "a"}}
    pdbs = [{"namespace": "default", "selector": pr.BROKEN[0], "disruptions_allowed": 0}, {"namespace": "default", "selector": None},
            {"namespace": "default", "selector": {}, "disruptions_allowed": 0}, {"namespace": "default", "selector": good, "disruptions_allowed": 9},
            {"namespace": "other", "selector": good, "disruptions_allowed": -3}]
    off, member = pdb.matching_members(pdbs, pods)
    assert off.tolist() == [0, 1, 2, 2] and member.tolist() == [3, 4]
    assert pdb.allowed_vector(pdbs).tolist() == [0, 0, 0, 9, -3]
    assert pdb.matching_members([], pods)[0].tolist() == [0, 0, 0, 0] and pdb.matching_members(pdbs, [])[0].tolist() == [0]
    assert pdb.allowed_vector([]).shape == (0,)


def test_hand_known_answers():
    kats = pr.hand_kats()
    assert len(kats) >= 8
    for sc in kats:
        m = pr.Model(sc["allowed"], sc["member_off"], sc["member"])
        assert m.bits(sc["ids"]).tolist() == sc["expect"], sc["name"]
        if "append" in sc:
            m.append(sc["append"]["member_off"], sc["append"]["member"])
        if "apply" in sc:
            m.allowed_apply(sc["apply"]["index"], sc["apply"]["value"])
        if "expect_after" in sc:
            assert m.bits(sc["ids"]).tolist() == sc["expect_after"], sc["name"] + " (after)"


def test_columns_follow_the_table():
    bits = np.array([1, 0, 1, 1, 0], np.uint8)
    col, nviol = pr.columns(bits, [4, 2, 0, 3], [0, 0, 2, 2], 4)             # id 1 is dead: its row is never visited
    assert col.tolist() == [0, 1, 1, 1] and nviol.tolist() == [1, 0, 2, 0]
    col, nviol = pr.columns(bits, [], [], 2)
    assert col.size == 0 and nviol.tolist() == [0, 0]


def _args(header: str, name: str) -> list:
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "bsched.h")).read()
    assert _args(header, "bs_pdb_load") == ["bs_ctx* ctx", "uint32_t n_pdb", "const int32_t* allowed", "uint32_t b", "const uint32_t* member_off",
                                            "const uint32_t* member"]
    assert _args(header, "bs_pdb_members_append") == ["bs_ctx* ctx", "uint32_t first_id", "uint32_t n", "const uint32_t* member_off", "const uint32_t* member"]
    assert _args(header, "bs_pdb_allowed_apply") == ["bs_ctx* ctx", "uint32_t count", "const uint32_t* index", "const int32_t* value"]
    assert _args(header, "bs_pdb_read") == ["bs_ctx* ctx", "uint32_t* n_pdb_out", "uint32_t* covered_out", "int32_t* allowed_out", "uint32_t* node_violating_out"]
    assert re.search(r"#define BS_PDB_MAX \(1u << 20\)", header) and re.search(r"#define BS_PDB_MEMBERS_MAX \(1u << 28\)", header)
    assert re.search(r"#define BS_ABI_VERSION 7u", header)
    for name in ("bs_pdb_load", "bs_pdb_members_append", "bs_pdb_allowed_apply", "bs_pdb_read"):
        assert name in capi.ABI_SYMBOLS, name
    lib = capi.load_library(bsa.build.build())
    vp, u32, P = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER
    pu, pi = P(ctypes.c_uint32), P(ctypes.c_int32)
    assert lib.bs_pdb_load.argtypes == [vp, u32, pi, u32, pu, pu]
    assert lib.bs_pdb_members_append.argtypes == [vp, u32, u32, pu, pu]
    assert lib.bs_pdb_allowed_apply.argtypes == [vp, u32, pu, pi]
    assert lib.bs_pdb_read.argtypes == [vp, pu, pu, pi, pu]
    assert lib.bs_pdb_load(None, 0, None, 0, None, None) == -1 and lib.bs_pdb_members_append(None, 0, 0, None, None) == -1
    assert lib.bs_pdb_allowed_apply(None, 0, None, None) == -1 and lib.bs_pdb_read(None, None, None, None, None) == -1
    assert lib.bs_abi_version() == 7
