"""The C ABI of bs_bound_bind (include/bsched.h): the declaration's argument list, capi.ABI_SYMBOLS and the binding, the exported symbol,
a NULL context refused, and the ABI version (the call is additive: it stays 7).  No GPU: nothing here creates a context."""
import ctypes as C
import importlib
import os
import re

bsa = importlib.import_module("batch-scheduler_amd")
capi = bsa.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bsched.h")).read()
ARGS = ["bs_ctx* ctx", "uint32_t n_wait", "const uint32_t* wait_id", "uint32_t n_pod", "const uint32_t* pod_index", "const int32_t* priority",
        "const int64_t* start_ns", "const uint8_t* pdb_violating", "uint32_t* node_out", "uint32_t* first_id_out"]


def test_the_declaration():
    m = re.search(r"\bint\s+bs_bound_bind\s*\(([^;]*?)\)\s*;", HEADER, re.S)
    assert m, "bs_bound_bind is not declared in include/bsched.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [re.sub(r"\s+", " ", a).strip() for a in args.split(",")] == ARGS
    assert re.search(r"#define\s+BS_ABI_VERSION\s+7u", HEADER)
    assert HEADER.index("int bs_bound_nodes_apply(") < m.start() < HEADER.index("resident PodDisruptionBudgets: the PDB bits follow"), "behind bs_bound_nodes_apply"


def test_the_header_states_the_rules():
    text = HEADER[HEADER.index("pods that leave Permit enter the bound table"):HEADER.index("int bs_bound_bind(")]
    for word in ("core.go:327", "bs_wait_park's rule", "all or nothing", "BS_ERR_STATE", "BS_ERR_INVALID", "BS_ERR_CAPACITY", "BS_BOUND_MAX_PER_NODE", "hazard",
                 "bs_seq_waiting_read", "first_id_out = ids"):
        assert word in text, word


def test_the_symbol_is_listed_bound_and_exported():
    assert "bs_bound_bind" in capi.ABI_SYMBOLS
    assert hasattr(bsa.Context, "bound_bind")
    lib = capi.load_library()
    assert hasattr(lib, "bs_bound_bind"), "libbsched.so does not export bs_bound_bind"
    assert len(lib.bs_bound_bind.argtypes) == len(ARGS)


def test_a_null_context_is_refused_and_the_abi_version_stays():
    lib = capi.load_library()
    assert lib.bs_abi_version() == 7
    first = C.c_uint32(0)
    assert lib.bs_bound_bind(None, 0, None, 0, None, None, None, None, None, C.byref(first)) == -1
