"""The C ABI of bs_preempt_commit_gang (include/bsched.h): the declarations with their argument lists, the exported symbols, a NULL
context refused, and the ABI version (the call is additive: it stays 7).  No GPU: nothing here creates a context."""
import ctypes as C
import importlib
import os
import re

bsa = importlib.import_module("batch-scheduler_amd")
capi = bsa.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bs_preempt_commit_gang", "bs_preempt_commit_gang_flat", "bs_preempt_gang_read")


def _decl(name: str) -> list:
    text = open(os.path.join(ROOT, "include", "bsched.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, f"{name} is not declared in include/bsched.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def test_declarations():
    assert _decl("bs_preempt_commit_gang") == [
        "bs_ctx* ctx", "uint32_t stages", "uint32_t count", "const uint32_t* pod_index", "const int32_t* priority",
        "const uint8_t* group_protected", "const uint32_t* gang_need", "uint32_t flags", "uint32_t victim_cap", "const bs_preempt_out* out"]
    flat, gang_flat = _decl("bs_preempt_commit_flat"), _decl("bs_preempt_commit_gang_flat")
    at = flat.index("const uint8_t* group_protected") + 1
    assert gang_flat == flat[:at] + ["const uint32_t* gang_need"] + flat[at:]        # bs_preempt_commit_flat's, gang_need after group_protected
    assert _decl("bs_preempt_gang_read") == ["bs_ctx* ctx", "uint32_t count", "uint8_t* slot_voided", "uint32_t g", "uint32_t* group_placed"]


def test_symbols_are_listed_and_exported():
    lib = capi.load_library()
    for name in NEW:
        assert name in capi.ABI_SYMBOLS, name
        assert getattr(lib, name) is not None
    assert len(lib.bs_preempt_commit_gang.argtypes) == 10 and len(lib.bs_preempt_commit_gang_flat.argtypes) == 16
    assert len(lib.bs_preempt_gang_read.argtypes) == 5


def test_null_context_is_refused_and_abi_version_stays():
    lib = capi.load_library()
    assert lib.bs_abi_version() == 7
    assert lib.bs_preempt_commit_gang(None, 1, 0, None, None, None, None, 0, 0, None) == -1
    assert lib.bs_preempt_commit_gang_flat(None, 1, 0, None, None, None, None, 0, 0, None, None, None, None, None, None, None) == -1
    assert lib.bs_preempt_gang_read(None, 0, None, 0, None) == -1
    for helper in ("gang_order", "gang_need"):
        assert callable(getattr(capi, helper))
    assert hasattr(bsa.Context, "preempt_commit_gang")
