"""csrc/bs_layouts.hpp, the layouts of the pod, group and result packs, compiled alone with tests/native/layouts_main.cpp under
ASan + UBSan and held against the rule written out here: the columns of each pack in order, with their element types; every piece at
the running offset rounded up to 256; max(n, 1) elements; `bytes` the final offset.  No GPU."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "batch-scheduler_amd", "csrc")

SIZES = (0, 1, 63, 64, 65, 257)
LANES = (1, 4, 8)


def pod_rule(P, L):
    n = max(P, 1)
    return [("group", "i4", n), ("req", "i8", n * L), ("pres", "u4", n), ("cls", "u4", n), ("owner", "u8", n), ("flags", "u1", n),
            "in_bytes", ("pclass", "u4", n), ("ppair", "u4", n), "bytes"]


def group_rule(G, L):
    n = max(G, 1)
    return [("mm", "u4", n), ("sc", "u4", n), ("matched", "u4", n), ("flags", "u1", n), ("cls", "u4", n), ("minres", "i8", n * L),
            ("mrpres", "u4", n), ("occ", "u8", n), "bytes"]


def out_rule(P, G):
    n, g = max(P, 1), max(G, 1)
    return [("pf_code", "u1", n), ("pf_first_k", "u4", n), ("pf_leader", "i4", n), ("fl_code", "u1", n), ("fl_feasible", "u4", n),
            ("fl_slot", "u4", n), ("admit", "u4", g), ("ready", "u1", g), "bytes"]


def test_pack_layouts_under_sanitizers(tmp_path):
    exe = str(tmp_path / "layouts")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "native", "layouts_main.cpp"), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1] == "OK"                                 # every piece's first and last element was stored inside `bytes`
    cols, totals = {}, {}
    for line in lines[:-1]:
        kind, pack, a, b, name, *v = line.split()
        key = (pack, int(a), int(b))
        if kind == "C":
            cols.setdefault(key, []).append((name, v[2], int(v[1]), int(v[0])))     # name, type, count, offset
        else:
            assert kind == "T", line
            totals.setdefault(key, {})[name] = int(v[0])
    want = {("pod", n, L): pod_rule(n, L) for n in SIZES for L in LANES}
    want.update({("group", n, L): group_rule(n, L) for n in SIZES for L in LANES})
    want.update({("out", P, G): out_rule(P, G) for P in SIZES for G in SIZES})
    assert sorted(cols) == sorted(totals) == sorted(want)
    for key, rule in want.items():
        got = iter(cols[key])
        o = 0                                                # the rule: a piece starts at the running offset, which then moves to its end rounded up to 256
        for step in rule:
            if isinstance(step, str):                        # a boundary or the total: the running offset where it stands
                assert totals[key][step] == o, (key, step)
                continue
            name, typ, n = step
            assert next(got) == (name, typ, n, o), (key, name)
            assert o % 256 == 0
            o = -(-(o + n * int(typ[1:])) // 256) * 256
        assert next(got, None) is None, key
    for (pack, a, b), t in totals.items():
        if pack == "pod":
            assert t["p"] == a and set(t) == {"in_bytes", "bytes", "p"}
        elif pack == "group":
            assert t["g"] == a and t["mark"] == t["bytes"] and set(t) == {"bytes", "mark", "g"}      # the carve started at 0: its mark is the pack's size
        else:
            assert set(t) == {"bytes"}


def test_the_header_is_host_only_and_the_context_holds_no_loose_layout_fields():
    """bs_layouts.hpp includes no HIP header (only bs_carve.hpp, <algorithm>, <stdint.h>); no source names a loose offset field of the
    group or result pack again, and bs_groups_load no longer keeps its own statement of group_layout's steps"""
    text = open(os.path.join(CSRC, "bs_layouts.hpp")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)", text)
    assert not [h for h in includes if "hip" in h]
    assert sorted(includes) == ["algorithm", "bs_carve.hpp", "stdint.h"]
    for name in sorted(os.listdir(CSRC)):
        src = open(os.path.join(CSRC, name)).read()
        for gone in ("off_gmm", "off_pf_code", "gpack_bytes", "outpack_bytes", "keeps its own statement"):
            assert gone not in src, (name, gone)
