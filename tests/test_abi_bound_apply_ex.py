"""bs_bound_apply_ex and bs_bound_apply_ex_flat are declared in include/bsched.h with the stated argument lists — the flags in front of
bs_bound_apply_flat's arguments, in its order —, are listed in capi.ABI_SYMBOLS with matching ctypes prototypes, BS_BOUND_NODES is 1 on
both sides, and BS_ABI_VERSION is still 7 (the change is additive)."""
import ctypes
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bsa = importlib.import_module("batch-scheduler_amd")
soa, capi = bsa.soa, bsa.capi


def _args(header: str, name: str) -> list:
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_entry_points_are_declared_with_the_stated_arguments():
    header = open(os.path.join(ROOT, "include", "bsched.h")).read()
    assert _args(header, "bs_bound_apply_ex") == ["bs_ctx* ctx", "const bs_bound_delta* delta", "uint32_t flags", "uint32_t* first_id_out"]
    flat, ex_flat = _args(header, "bs_bound_apply_flat"), _args(header, "bs_bound_apply_ex_flat")
    assert ex_flat == [flat[0], "uint32_t flags"] + flat[1:]
    assert _args(header, "bs_bound_apply") == ["bs_ctx* ctx", "const bs_bound_delta* delta", "uint32_t* first_id_out"]      # as it was
    assert re.search(r"#define BS_BOUND_NODES 1u\b", header)
    assert re.search(r"#define BS_ABI_VERSION 7u", header)


def test_binding_lists_them():
    for name in ("bs_bound_apply_ex", "bs_bound_apply_ex_flat", "bs_bound_apply", "bs_bound_apply_flat"):
        assert name in capi.ABI_SYMBOLS, name
    assert capi.BS_BOUND_NODES == 1 and soa.BS_BOUND_NODES == 1


def test_library_exports_them_and_refuses_a_null_context():
    lib = capi.load_library(bsa.build.build())
    u32 = ctypes.c_uint32
    assert lib.bs_bound_apply_ex.argtypes[2] is u32 and len(lib.bs_bound_apply_ex.argtypes) == 4
    assert lib.bs_bound_apply_ex_flat.argtypes == [lib.bs_bound_apply_flat.argtypes[0], u32] + lib.bs_bound_apply_flat.argtypes[1:]
    d = soa.BoundDeltaStruct()
    assert lib.bs_bound_apply_ex(None, ctypes.byref(d), 1, None) == -1
    assert lib.bs_bound_apply_ex_flat(None, 1, 0, None, 0, None, None, None, None, None, None, None, None) == -1
    assert lib.bs_abi_version() == 7
