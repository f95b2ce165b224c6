"""CPU tests of bs_groups_list_apply's statement: the array model (tests/groups_list_ref.py) against a naive object-by-object rebuild over
random deltas, the host check header (csrc/bs_groups_list_check.hpp) as a stand-alone program under ASan + UBSan against the model, hand-written
known answers, and the new translation unit's place in the build.  No GPU."""
import importlib
import json
import os
import subprocess
from types import SimpleNamespace

import numpy as np

import groups_list_ref as gl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


class Rows(SimpleNamespace):
    """the eight columns of bs_groups_soa, numpy only"""

    def __init__(self, *cols):
        super().__init__(**dict(zip(gl.COLUMNS, cols)))


def rows_named(names, L=5):
    """one row per name: every column is a function of the name, so a row can be recognised wherever it ends up"""
    k = np.array([ord(c) for c in names], np.int64)
    return Rows((k % 7 + 1).astype(np.uint32), (k % 3).astype(np.uint32), (k % 5).astype(np.uint32), (k % 16).astype(np.uint8), (k % 4).astype(np.uint32),
                (np.arange(L)[:, None] * 1000 + k[None, :]).astype(np.int64), (k % 2).astype(np.uint32), (k * 11).astype(np.uint64))


def names_of(rows):
    return "".join(chr(int(x) // 11) for x in rows.occupied_by)


# ---- the model against the naive rebuild ----------------------------------------------------------------------------------------------------------
def test_the_model_equals_an_object_by_object_rebuild():
    rng = np.random.default_rng(2026)
    letters = [chr(c) for c in range(0x100, 0x100 + 400)]
    seen = dict(remove_all=0, both=0, from_zero=0, append_only=0, dropped=0)
    for case in range(300):
        g = int(rng.integers(0, 40)) if case % 10 else 0
        names = "".join(letters[:g])
        remove, update, rows, n_append = gl.random_delta(rng, g, lambda k: rows_named("".join(letters[100 + case % 50: 100 + case % 50 + k])))
        if case % 7 == 0 and remove and not update:
            update = remove[:1]
            rows = rows_named("".join(letters[200: 200 + 1 + n_append]))
        hi = g + 3
        pods = rng.integers(-2, hi, int(rng.integers(0, 60))).astype(np.int32)
        bound = rng.integers(-2, hi, int(rng.integers(0, 30))).astype(np.int32)
        w = int(rng.integers(0, 50)) if g else 0
        wait = dict(id=np.sort(rng.choice(1000, w, replace=False)).astype(np.uint32), node=rng.integers(0, 9, w).astype(np.uint32),
                    group=rng.integers(0, max(g, 1), w).astype(np.int32), req=rng.integers(0, 99, (5, w)).astype(np.int64), req_present=rng.integers(0, 2, w).astype(np.uint32))
        leader = int(rng.integers(-1, g + 1))
        assert gl.check(g, remove, update, rows.min_member.size, n_append) == gl.OK
        m = gl.list_apply(rows_named(names), remove, update, rows, pods, bound, wait, leader, make=Rows)
        new_names = names_of(rows)
        n_rows, n_pods, n_bound, kept, dropped = gl.naive(list(names), remove, update, list(new_names), pods.tolist(), bound.tolist(),
                                                          list(zip(wait["id"].tolist(), wait["node"].tolist(), wait["group"].tolist())))
        assert names_of(m["groups"]) == "".join(n_rows) and m["g_new"] == len(n_rows) == g - len(remove) + n_append
        want = rows_named("".join(n_rows))
        for name in gl.COLUMNS:
            assert np.array_equal(getattr(m["groups"], name), getattr(want, name)), (case, name)
        assert m["pod_group"].tolist() == n_pods and m["bound_group"].tolist() == n_bound
        assert m["n_pods_missing"] == sum(1 for a, b in zip(pods.tolist(), n_pods) if b == -2 and a != -2)
        assert m["n_bound_missing"] == sum(1 for a, b in zip(bound.tolist(), n_bound) if b == -2 and a != -2)
        assert list(zip(m["wait"]["id"].tolist(), m["wait"]["node"].tolist(), m["wait"]["group"].tolist())) == kept
        assert list(zip(*[c.tolist() for c in m["dropped"]])) == dropped
        keep = np.isin(wait["id"], m["wait"]["id"])
        assert np.array_equal(m["wait"]["req"], wait["req"][:, keep]) and np.array_equal(m["wait"]["req_present"], wait["req_present"][keep])
        led = gl.naive(list(names), remove, update, list(new_names), [leader], [], [])[1][0]     # the leader as one more reference to a group
        assert m["leader"] == (-1 if led == gl.MISSING else led)
        assert gl.max_group(leader, g, remove) >= m["leader"] or leader >= g
        seen["remove_all"] += bool(g and len(remove) == g)
        seen["both"] += bool(set(remove) & set(update))
        seen["from_zero"] += bool(g == 0 and n_append)
        seen["append_only"] += bool(not remove and not update and n_append)
        seen["dropped"] += bool(dropped)
    assert all(v >= 5 for v in seen.values()), seen


# ---- the check header alone, under sanitizers -----------------------------------------------------------------------------------------------------
def test_the_check_header_under_sanitizers(tmp_path):
    """csrc/bs_groups_list_check.hpp compiled alone with tests/native/groups_list_main.cpp under ASan + UBSan; the program is run directly"""
    exe = str(tmp_path / "groups_list")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "batch-scheduler_amd", "csrc"), os.path.join(HERE, "native", "groups_list_main.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(77)
    lines, want, codes = [], [], []

    def add(g, mask, remove, update, rows_g, n_append, wait_cap):
        lines.append(" ".join(map(str, [g, mask, len(remove), *remove, len(update), *update, rows_g, n_append, wait_cap])))
        code = gl.check(g, remove, update, rows_g, n_append, rows_null=bool(mask & 4), wait_cap=wait_cap, wait_null=bool(mask & 8),
                        remove_null=bool(mask & 1), update_null=bool(mask & 2))
        codes.append(code)
        if code != gl.OK:
            want.append([code])
            return
        imap = gl.index_map(g, remove)
        want.append([0, g - len(remove) + n_append, *imap.tolist(), *[gl.max_group(m, g, remove) for m in range(-1, g + 1)]])
    # the edges by hand: an empty delta, remove all, g = 0 -> append, an index both updated and removed
    add(5, 0, [], [], 0, 0, 0)
    add(0, 0, [], [], 0, 0, 0)
    add(6, 0, [0, 1, 2, 3, 4, 5], [], 0, 0, 0)
    add(0, 0, [], [], 3, 3, 0)
    add(4, 0, [1], [1, 3], 2, 0, 0)
    add(1, 0, [0], [0], 4, 3, 7)
    # every error
    add(3, 0, [3], [], 0, 0, 0)                    # a remove index at g
    add(3, 0, [], [7], 1, 0, 0)                    # an update index above g
    add(0, 0, [0], [], 0, 0, 0)                    # any index on an empty list
    add(4, 0, [2, 1], [], 0, 0, 0)                 # not ascending
    add(4, 0, [2, 2], [], 0, 0, 0)                 # not STRICTLY ascending
    add(4, 0, [], [0, 3, 3], 3, 0, 0)
    add(4, 0, [], [1], 0, 0, 0)                    # rows.g too small
    add(4, 0, [], [], 2, 1, 0)                     # rows.g too large
    add(4, 0, [], [], 0, 0xFFFFFFFF, 0)            # (the sum does not wrap)
    add(4, 1, [1], [], 0, 0, 0)                    # NULL remove
    add(4, 2, [], [1], 1, 0, 0)                    # NULL update
    add(4, 4, [], [], 1, 1, 0)                     # a NULL column of rows
    add(4, 8, [], [], 0, 0, 5)                     # a NULL result array with a cap
    add(4, 15, [], [], 0, 0, 0)                    # NULL everywhere with every count and cap 0: fine
    add(3, 0, [5, 1], [], 0, 0, 0)                 # range before order, entry by entry
    add(3, 0, [1, 0, 9], [], 0, 0, 0)              # ... and order where it comes first
    for _ in range(400):
        g = int(rng.integers(0, 12))
        if rng.random() < 0.6:
            remove, update, rows, n_append = gl.random_delta(rng, g, lambda k: rows_named("x" * k))
            rows_g = rows.min_member.size
        else:                                       # lists that may be out of range, unsorted or repeated; a row count that may be off
            remove = rng.integers(0, g + 2, int(rng.integers(0, 5))).tolist()
            update = rng.integers(0, g + 2, int(rng.integers(0, 4))).tolist()
            if rng.random() < 0.5:
                remove, update = sorted(set(remove)), sorted(set(update))
            n_append = int(rng.integers(0, 4))
            rows_g = len(update) + n_append + int(rng.random() < 0.2)
        mask = int(rng.integers(0, 16)) if rng.random() < 0.25 else 0
        add(g, mask, remove, update, rows_g, n_append, int(rng.integers(0, 3)))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(want)
    for line, got, exp in zip(lines, out, want):
        assert [int(x) for x in got.split()] == exp, line
    assert all(codes.count(c) >= 5 for c in (gl.OK, gl.E_NULL, gl.E_ROWS, gl.E_RANGE, gl.E_ORDER)), [codes.count(c) for c in range(5)]


# ---- known answers by hand ---------------------------------------------------------------------------------------------------------------------------
def test_hand_written_known_answers():
    kats = json.load(open(os.path.join(HERE, "golden", "groups_list_hand_kats.json")))["cases"]
    assert len(kats) >= 5
    for k in kats:
        wait = k["wait"]
        tab = dict(id=np.array([r[0] for r in wait], np.uint32), node=np.array([r[1] for r in wait], np.uint32), group=np.array([r[2] for r in wait], np.int32),
                   req=np.arange(5 * len(wait), dtype=np.int64).reshape(5, len(wait)), req_present=np.zeros(len(wait), np.uint32))
        assert gl.check(len(k["groups"]), k["remove"], k["update"], len(k["rows"]), k["n_append"]) == gl.OK, k["name"]
        m = gl.list_apply(rows_named(k["groups"]), k["remove"], k["update"], rows_named(k["rows"]), np.array(k["pods"], np.int32), np.array(k["bound"], np.int32),
                          tab, k["leader"], make=Rows)
        w = k["want"]
        assert names_of(m["groups"]) == w["groups"] and m["g_new"] == len(w["groups"]), k["name"]
        assert m["map"].tolist() == w["map"], k["name"]
        assert m["pod_group"].tolist() == w["pods"] and m["n_pods_missing"] == w["n_pods_missing"], k["name"]
        assert m["bound_group"].tolist() == w["bound"] and m["n_bound_missing"] == w["n_bound_missing"], k["name"]
        assert [list(r) for r in zip(m["wait"]["id"].tolist(), m["wait"]["node"].tolist(), m["wait"]["group"].tolist())] == w["wait"], k["name"]
        assert [list(r) for r in zip(*[c.tolist() for c in m["dropped"]])] == w["dropped"], k["name"]
        assert m["leader"] == w["leader"] and gl.max_group(k["max_group"], len(k["groups"]), k["remove"]) == w["max_group"], k["name"]


# ---- the new unit's place in the build ------------------------------------------------------------------------------------------------------------------
def test_the_groups_unit_is_built_linked_and_lists_every_header_it_reaches():
    build = importlib.import_module("batch-scheduler_amd.build")
    from test_build_units_cpu import closure, MAIN_HEADERS
    assert "tu_groups.hip" in build.SOURCES
    assert set(build.HEADERS) >= {"bs_groups_list.hpp", "bs_groups_list_check.hpp"}
    reached = closure("tu_groups.hip")
    assert not reached - {os.path.normpath(h) for h in build.UNITS["tu_groups.hip"]}, sorted(reached)
    assert {"bs_groups_list.hpp", "bs_groups_list_check.hpp"} <= reached and not MAIN_HEADERS & reached
    assert not {"bs_wait.hpp", "bs_seq.hpp"} & reached, "the unit reaches the wait table through bs_ctx.hpp's two declarations only"
    for unit in ("bsched.hip", "tu_seq.hip", "tu_wait.hip"):
        assert not {"bs_groups_list.hpp"} & closure(unit), unit
    assert '#include "tu_groups.hip"' in open(os.path.join(build.CSRC, "bsched.hip")).read(), "the unity build includes the unit"
    check = open(os.path.join(build.CSRC, "bs_groups_list_check.hpp")).read()
    assert "#include <hip" not in check and "__global__" not in check and "__device__" not in check, "the check header is plain C++"


def test_the_kernels_use_no_scratch_and_live_in_a_unit_of_their_own():
    """k_gl_gather<S>, S = 0..12, and k_gl_remap: no scratch, one unit, and that unit emits neither k_seq_pass nor a k_wt_* kernel"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    all_k = kernel_resources.resources()
    res = {k: v for k, v in all_k.items() if "k_gl_" in k}
    assert len(res) == 13 + 1, sorted(res)
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in res.values()), res
    units = {v["unit"] for v in res.values()}
    assert len(units) == 1 and units.isdisjoint({v["unit"] for k, v in all_k.items() if "k_seq_pass" in k or "k_wt_" in k or "k_se_" in k})
