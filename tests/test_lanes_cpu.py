"""csrc/bs_lanes.hpp, the three rules by which a context's scalar-lane count picks a kernel instantiation, compiled alone with
tests/native/lanes_main.cpp under ASan + UBSan and held against the rules written out here.  No GPU."""
import importlib
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "batch-scheduler_amd", "csrc")
build = importlib.import_module("batch-scheduler_amd.build")


def test_the_three_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lanes")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "native", "lanes_main.cpp"), "-o", exe], check=True)
    rows = [[int(x) for x in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(41))
    for S, wide, wide_calls, narrow, narrow_calls, clamped, clamped_calls, ret_wide, ret_narrow, ret_clamped in rows:
        assert (wide_calls, narrow_calls, clamped_calls) == (1, 1, 1), S
        assert wide == min(S, 12), S
        assert narrow == (S if S <= 4 else -1), S
        assert clamped == min(S, 4), S
        # a callable that returns a value: the same constant comes back through the rule
        assert (ret_wide, ret_narrow, ret_clamped) == (1000 + wide, 1000 + narrow, 1000 + clamped), S


def test_the_header_is_host_only_and_no_host_switch_on_the_lane_count_is_left():
    """bs_lanes.hpp includes no HIP header; no `switch` on S / c->S / c.S / ts remains in the host code of the translation units"""
    text = open(os.path.join(CSRC, "bs_lanes.hpp")).read()
    assert not [h for h in re.findall(r"#include\s*[<\"]([^>\"]+)", text) if "hip" in h]
    for unit in build.SOURCES + ["bs_ctx.hpp", "bs_bound_cols.hpp"]:
        src = open(os.path.join(CSRC, unit)).read()
        assert not re.search(r"switch\s*\(\s*(S|c->S|c\.S|ts)\b", src), unit
