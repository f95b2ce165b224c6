"""The C ABI of bs_seq_run_scored, its flat form and bs_seq_score_read (include/bsched.h): the declarations with their argument lists against
the ctypes prototypes, the exported symbols, bs_seq_score and BS_SCORE_WEIGHT_MAX, the flat form as bs_seq_run_flat's result arguments behind
the three weights, a NULL context refused, rule P, P1 and P2 stated in the header, and the ABI version (the calls are additive: it stays
7).  No GPU: nothing here creates a context."""
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
    "bs_seq_run_scored": ["bs_ctx* ctx", "uint32_t stages", "const bs_seq_score* score", "bs_seq_out* out"],
    "bs_seq_score_read": ["bs_ctx* ctx", "uint32_t p", "uint32_t* total", "uint32_t* n_fit"],
    "bs_seq_run_scored_flat": ["bs_ctx* ctx", "uint32_t stages", "uint32_t w_least", "uint32_t w_most", "uint32_t w_balanced"] + FLAT_RESULTS,
}


def _ctype(name):
    return {"bs_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "uint32_t*": C.POINTER(C.c_uint32), "int32_t*": C.POINTER(C.c_int32), "uint8_t*": C.POINTER(C.c_uint8),
            "int64_t*": C.POINTER(C.c_int64), "bs_seq_out*": C.POINTER(capi.SeqOut), "const bs_seq_score*": C.POINTER(capi.SeqScore)}[name]


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
    assert _decl("bs_seq_run_flat")[2:] == FLAT_RESULTS == _decl("bs_seq_run_scored_flat")[5:], "the flat form mirrors bs_seq_run_flat's result arguments"
    assert re.search(r"#define\s+BS_SCORE_WEIGHT_MAX\s+65536u", HEADER) and capi.SCORE_WEIGHT_MAX == 65536
    assert re.search(r"typedef struct bs_seq_score \{ uint32_t w_least, w_most, w_balanced; \} bs_seq_score;", HEADER)
    assert [f[0] for f in capi.SeqScore._fields_] == ["w_least", "w_most", "w_balanced"] and C.sizeof(capi.SeqScore) == 12
    for meth in ("seq_run_scored", "seq_score_read"):
        assert hasattr(bsa.Context, meth), meth


def test_the_header_states_the_rule():
    for words in ("D7. (rule P;", "Library rule P1:", "Library rule P2:", "0 < A < 2^53 and 0 <= R <= A", "ties to the LOWEST node index", "NonZeroRequest",
                  "least_j = ((A - R) * 100) / A", "every operation rounded on its own", "selectHost", "Out of scope: the scored choice together with the nominated-pod table"):
        assert words in HEADER, words
    assert HEADER.index("int bs_seq_nominated_read") < HEADER.index("D7. (rule P;") < HEADER.index("int bs_seq_run_scored("), "the section sits behind bs_seq_run_nominated"


def test_null_context_is_refused_and_abi_version_stays():
    lib = capi.load_library()
    assert lib.bs_abi_version() == 7 and re.search(r"#define\s+BS_ABI_VERSION\s+7u", HEADER)
    o, w = capi.SeqOut(), capi.SeqScore(1, 0, 1)
    assert lib.bs_seq_run_scored(None, 1, C.byref(w), C.byref(o)) == -1
    assert lib.bs_seq_run_scored_flat(None, 1, 1, 0, 1, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.bs_seq_score_read(None, 0, None, None) == -1
