"""The C ABI of bs_seq_run_scored_nominated and its flat form (include/bsched.h): the declarations with their argument lists against the
ctypes prototypes, the exported symbols, the flat form as bs_seq_run_nominated_flat's two arrays and bs_seq_run_scored_flat's three weights in
front of bs_seq_run_flat's result arguments, a NULL context refused, rule SP, D8, SP1 and SP2 stated in the header, and the ABI version (the
calls are additive: it stays 7).  No GPU: nothing here creates a context."""
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
CALL = ["bs_ctx* ctx", "uint32_t stages", "uint32_t p", "const int32_t* priority", "const uint32_t* own_id"]
WEIGHTS = ["uint32_t w_least", "uint32_t w_most", "uint32_t w_balanced"]
DECLS = {
    "bs_seq_run_scored_nominated": CALL + ["const bs_seq_score* score", "bs_seq_out* out"],
    "bs_seq_run_scored_nominated_flat": CALL + WEIGHTS + FLAT_RESULTS,
}


def _ctype(name):
    return {"bs_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "uint32_t*": C.POINTER(C.c_uint32), "const uint32_t*": C.POINTER(C.c_uint32),
            "int32_t*": C.POINTER(C.c_int32), "const int32_t*": C.POINTER(C.c_int32), "uint8_t*": C.POINTER(C.c_uint8), "int64_t*": C.POINTER(C.c_int64),
            "bs_seq_out*": C.POINTER(capi.SeqOut), "const bs_seq_score*": C.POINTER(capi.SeqScore)}[name]


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
        assert getattr(lib, name).argtypes == [_ctype(a.rsplit(" ", 1)[0]) for a in args], name
    flat = _decl("bs_seq_run_scored_nominated_flat")
    assert flat[:5] == _decl("bs_seq_run_nominated_flat")[:5] and flat[5:8] == _decl("bs_seq_run_scored_flat")[2:5], "the two parents' arguments, in that order"
    assert flat[8:] == FLAT_RESULTS == _decl("bs_seq_run_flat")[2:], "the flat form mirrors bs_seq_run_flat's result arguments"
    assert hasattr(bsa.Context, "seq_run_scored_nominated")


def test_the_header_states_the_rule():
    for words in ("SP. (rule SP.)", "D8. (recalled upstream, v1.17.5, not vendored.)", "Library rule SP1:", "Library rule SP2:", "No row enters a score",
                  "addNominatedPods works on a COPY of the NodeInfo", "PrioritizeNodes reads the snapshot", "ties to the LOWEST node index",
                  "the allocatable key still required", "bs_nominated_load with m = 0"):
        assert words in HEADER, words
    assert HEADER.index("int bs_seq_score_read") < HEADER.index("SP. (rule SP.)") < HEADER.index("int bs_seq_run_scored_nominated("), "the section sits behind bs_seq_run_scored"
    assert HEADER.index("D7. (rule P;") < HEADER.index("D8. (recalled upstream")


def test_null_context_is_refused_and_abi_version_stays():
    lib = capi.load_library()
    assert lib.bs_abi_version() == 7 and re.search(r"#define\s+BS_ABI_VERSION\s+7u", HEADER)
    o, w = capi.SeqOut(), capi.SeqScore(1, 0, 1)
    assert lib.bs_seq_run_scored_nominated(None, 1, 0, None, None, C.byref(w), C.byref(o)) == -1
    assert lib.bs_seq_run_scored_nominated_flat(None, 1, 0, None, None, 1, 0, 1, None, None, None, None, 0, None, None, None, None, None, None) == -1
