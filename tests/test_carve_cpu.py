"""csrc/bs_carve.hpp, the running offset that hands out the typed pieces of every host-side scratch layout, compiled alone with
tests/native/carve_main.cpp under ASan + UBSan and held against the rule written out here.  No GPU."""
import importlib
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "batch-scheduler_amd", "csrc")
build = importlib.import_module("batch-scheduler_amd.build")


def test_offsets_and_totals_under_sanitizers(tmp_path):
    exe = str(tmp_path / "carve")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "native", "carve_main.cpp"), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[-1] == "OK"                                 # in(nullptr) is null, no piece overlaps, every first / last element was stored
    runs, totals = {}, {}
    for line in lines[:-1]:
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == "P":
            runs.setdefault((v[0], v[1]), []).append(v[2:])
        else:
            assert kind == "T", line
            totals[(v[0], v[1])] = v[2]
    assert sorted(runs) == sorted(totals) == [(pad, r) for pad in (1, 256) for r in range(7)]
    seen = set()
    for (pad, r), pieces in runs.items():
        o = 0                                                # the rule: a piece starts at the running offset, which then moves to its end rounded up to pad
        for size, n, off, nbytes in pieces:
            assert off == o and nbytes == n * size, (pad, r, size, n)
            o = -(-(o + n * size) // pad) * pad
            seen.add((pad, size, n))
        assert totals[(pad, r)] == o, (pad, r)
        if pad == 256:
            assert all(off % 256 == 0 for _, _, off, _ in pieces)
    # every element width met every count under both paddings (an empty piece takes no bytes: the rule above with n = 0)
    assert {(s, n) for p, s, n in seen if p == 256} == {(s, n) for p, s, n in seen if p == 1} == {(s, n) for s in (1, 4, 8, 24) for n in (0, 1, 63, 64, 65, 257, 1000)}


def test_the_header_is_host_only_and_no_hand_written_offset_table_is_left():
    """bs_carve.hpp includes no HIP header; the host code (every translation unit, bs_ctx.hpp and bs_bound_cols.hpp) no longer advances an offset by hand, and
    casts no `base + o_x` / `base + c->blay.x`, a base written as `buf.as<uint8_t>()` included"""
    text = open(os.path.join(CSRC, "bs_carve.hpp")).read()
    assert not [h for h in re.findall(r"#include\s*[<\"]([^>\"]+)", text) if "hip" in h]
    cast = r"reinterpret_cast<[^>]*>\(\s*[\w.<>()\-]+\s*\+\s*(?:o_\w+|c->blay\.\w*)"
    assert re.findall(cast, "reinterpret_cast<int32_t*>(c->d_bound.as<uint8_t>() + c->blay.group)")      # (the form the narrower pattern let through)
    for unit in build.SOURCES + ["bs_ctx.hpp", "bs_bound_cols.hpp"]:
        src = open(os.path.join(CSRC, unit)).read()
        assert "o = align256(o +" not in src, unit
        assert not re.findall(cast, src), unit
