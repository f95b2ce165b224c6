"""The ctypes structure of bs_bound_apply (soa.BoundDeltaStruct) against include/bsched.h, field by field, the way
tests/test_abi_layout.py checks its pairs; and the new entry points are declared in the header and in capi.ABI_SYMBOLS."""
import ctypes
import importlib
import os
import re
import subprocess

from test_abi_layout import _c_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bsa = importlib.import_module("batch-scheduler_amd")
soa, capi = bsa.soa, bsa.capi

PAIRS = [("bs_bound_delta", soa.BoundDeltaStruct)]


def test_bound_delta_matches_the_header(tmp_path):
    header = open(os.path.join(ROOT, "include", "bsched.h")).read()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "bsched.h"', "int main(void) {"]
    for cname, _ in PAIRS:
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f in _c_fields(header, cname):
            lines.append(f'  printf("{cname} {f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c_layout = {}
    for ln in out.splitlines():
        p = ln.split()
        if p[1] == "size":
            c_layout.setdefault(p[0], {})["__size__"] = int(p[2])
        else:
            c_layout.setdefault(p[0], {})[p[1]] = (int(p[2]), int(p[3]))
    for cname, ct in PAIRS:
        c = c_layout[cname]
        assert c["__size__"] == ctypes.sizeof(ct), cname
        names = [f for f, _ in ct._fields_]
        assert names == _c_fields(header, cname), f"{cname}: field order"
        for f in names:
            d = getattr(ct, f)
            assert (d.offset, d.size) == c[f], f"{cname}.{f}: ctypes {(d.offset, d.size)} vs C {c[f]}"


def test_bound_apply_entry_points_are_declared():
    header = open(os.path.join(ROOT, "include", "bsched.h")).read()
    for name in ("bs_bound_apply", "bs_bound_apply_flat", "bs_bound_ids", "bs_bound_dump"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.ABI_SYMBOLS, name
    assert re.search(r"#define BS_ABI_VERSION 7u", header)
