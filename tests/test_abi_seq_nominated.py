"""The C ABI of bs_seq_run_nominated, its flat form and bs_seq_nominated_read (include/bsched.h): the declarations with their argument lists
against the ctypes prototypes, the exported symbols, BS_NOM_NONE, the flat form as bs_seq_run_flat's arguments plus the call's two arrays, a
NULL context refused, rule S and D6 stated in the header, and the ABI version (the calls are additive: it stays 7).  No GPU: nothing here
creates a context."""
import ctypes as C
import importlib
import os
import re

bsa = importlib.import_module("batch-scheduler_amd")
capi = bsa.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bsched.h")).read()
FLAT_RESULTS = ["uint8_t* pf_code", "uint32_t* pf_first_k", "int32_t* pf_leader", "int32_t* pod_node", "uint32_t cap", "uint32_t* released_group",
                "uint32_t* released_pods", "int64_t* first_ns", "int64_t* ready_ns", "int64_t* scalars_out", "uint8_t* last_permitted"]
DECLS = {
    "bs_seq_run_nominated": ["bs_ctx* ctx", "uint32_t stages", "uint32_t p", "const int32_t* priority", "const uint32_t* own_id", "bs_seq_out* out"],
    "bs_seq_nominated_read": ["bs_ctx* ctx", "uint32_t cap", "uint32_t* id", "uint32_t* pod", "uint32_t* node", "uint32_t* n_out"],
    "bs_seq_run_nominated_flat": ["bs_ctx* ctx", "uint32_t stages", "uint32_t p", "const int32_t* priority", "const uint32_t* own_id"] + FLAT_RESULTS,
}
CTYPE = {"bs_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "const int32_t*": C.POINTER(C.c_int32), "const uint32_t*": C.POINTER(C.c_uint32),
         "uint32_t*": C.POINTER(C.c_uint32), "int32_t*": C.POINTER(C.c_int32), "uint8_t*": C.POINTER(C.c_uint8), "int64_t*": C.POINTER(C.c_int64),
         "bs_seq_out*": C.POINTER(capi.SeqOut)}


def _decl(name: str) -> list:
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, re.S)
    assert m, f"{name} is not declared in include/bsched.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def test_declarations_match_the_binding():
    lib = capi.load_library()
    for name, args in DECLS.items():
        assert _decl(name) == args, name
        assert name in capi.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes == [CTYPE[a.rsplit(" ", 1)[0]] for a in args], name
    assert _decl("bs_seq_run_flat")[2:] == FLAT_RESULTS, "the flat form mirrors bs_seq_run_flat's arguments"
    assert re.search(r"#define\s+BS_NOM_NONE\s+0xFFFFFFFFu", HEADER) and capi.NOM_NONE == 0xFFFFFFFF
    for meth in ("seq_run_nominated", "seq_nominated_read"):
        assert hasattr(bsa.Context, meth), meth


def test_the_header_states_the_rule():
    for words in ("(rule S.)", "D6.", "DeleteNominatedPodIfExists", "Library rule S1: PreFilter is untouched", "equal priority counts",
                  "that is not pod i's own row"):
        assert words in HEADER, words
    assert "keeps BS_PREEMPT_ASSUME" not in HEADER, "the clause that sent callers to BS_PREEMPT_ASSUME is gone"


def test_null_context_is_refused_and_abi_version_stays():
    lib = capi.load_library()
    assert lib.bs_abi_version() == 7 and re.search(r"#define\s+BS_ABI_VERSION\s+7u", HEADER)
    n = C.c_uint32(0)
    o = capi.SeqOut()
    assert lib.bs_seq_run_nominated(None, 1, 0, None, None, C.byref(o)) == -1
    assert lib.bs_seq_run_nominated_flat(None, 1, 0, None, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.bs_seq_nominated_read(None, 0, None, None, None, C.byref(n)) == -1
