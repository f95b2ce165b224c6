"""The C ABI of the two sampled passes (include/bsched.h): bs_seq_sample_size, bs_seq_run_scored_sampled, bs_seq_run_scored_nominated_sampled,
their flat forms and bs_seq_sample_read — the declarations with their argument lists against the ctypes prototypes, the exported symbols, the
flat forms as their parents' flat arguments with num_to_find and start behind the weights, a NULL context refused, rule F, D9, F1 to F3 and
the reason BS_BATCH_FILTER_DENY is refused stated in the header, and the ABI version (the calls are additive: it stays 7).  No GPU: nothing
here creates a context."""
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
HEAD = ["bs_ctx* ctx", "uint32_t stages"]
NOM = ["uint32_t p", "const int32_t* priority", "const uint32_t* own_id"]
WEIGHTS = ["uint32_t w_least", "uint32_t w_most", "uint32_t w_balanced"]
SAMPLE = ["uint32_t num_to_find", "uint32_t start"]
DECLS = {
    "bs_seq_run_scored_sampled": HEAD + ["const bs_seq_score* score", "const bs_seq_sample* sample", "bs_seq_out* out"],
    "bs_seq_run_scored_nominated_sampled": HEAD + NOM + ["const bs_seq_score* score", "const bs_seq_sample* sample", "bs_seq_out* out"],
    "bs_seq_run_scored_sampled_flat": HEAD + WEIGHTS + SAMPLE + FLAT_RESULTS,
    "bs_seq_run_scored_nominated_sampled_flat": HEAD + NOM + WEIGHTS + SAMPLE + FLAT_RESULTS,
    "bs_seq_sample_read": ["bs_ctx* ctx", "uint32_t p", "uint32_t* start", "uint32_t* visited", "uint32_t* next_start"],
}


def _ctype(name):
    return {"bs_ctx*": C.c_void_p, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint32_t*": C.POINTER(C.c_uint32), "const uint32_t*": C.POINTER(C.c_uint32),
            "int32_t*": C.POINTER(C.c_int32), "const int32_t*": C.POINTER(C.c_int32), "uint8_t*": C.POINTER(C.c_uint8), "int64_t*": C.POINTER(C.c_int64),
            "bs_seq_out*": C.POINTER(capi.SeqOut), "const bs_seq_score*": C.POINTER(capi.SeqScore), "const bs_seq_sample*": C.POINTER(capi.SeqSample)}[name]


def _decl(name: str, ret: str = "int") -> list:
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, re.S)
    assert m, f"{name} is not declared in include/bsched.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")]


def test_declarations_match_the_binding():
    lib = capi.load_library()
    for name, args in DECLS.items():
        assert _decl(name) == args, name
        assert name in capi.ABI_SYMBOLS, name
        assert getattr(lib, name).argtypes == [_ctype(a.rsplit(" ", 1)[0]) for a in args], name
        assert getattr(lib, name).restype is C.c_int, name
    assert _decl("bs_seq_sample_size", "uint32_t") == ["uint32_t n", "int32_t percentage"] and "bs_seq_sample_size" in capi.ABI_SYMBOLS
    assert lib.bs_seq_sample_size.argtypes == [C.c_uint32, C.c_int32] and lib.bs_seq_sample_size.restype is C.c_uint32
    assert re.search(r"typedef struct bs_seq_sample \{ uint32_t num_to_find; uint32_t start; \} bs_seq_sample;", HEADER)
    assert [f[0] for f in capi.SeqSample._fields_] == ["num_to_find", "start"] and C.sizeof(capi.SeqSample) == 8
    for name in ("seq_run_scored_sampled", "seq_run_scored_nominated_sampled", "seq_sample_read"):
        assert hasattr(bsa.Context, name), name
    assert callable(capi.seq_sample_size)


def test_the_flat_forms_carry_their_parents_arguments_with_the_sample_behind_the_weights():
    plain, parent = _decl("bs_seq_run_scored_sampled_flat"), _decl("bs_seq_run_scored_flat")
    assert plain[:5] == parent[:5] and plain[5:7] == SAMPLE and plain[7:] == parent[5:] == FLAT_RESULTS
    nom, parent = _decl("bs_seq_run_scored_nominated_sampled_flat"), _decl("bs_seq_run_scored_nominated_flat")
    assert nom[:8] == parent[:8] and nom[8:10] == SAMPLE and nom[10:] == parent[8:] == FLAT_RESULTS
    assert FLAT_RESULTS == _decl("bs_seq_run_flat")[2:], "the flat forms mirror bs_seq_run_flat's result arguments"


def test_the_header_states_the_rule():
    for words in ("D9. (recalled upstream, v1.17.5, not vendored: numFeasibleNodesToFind.)", "F. (rule F.)", "Library rule F1:", "Library rule F2:", "Library rule F3:",
                  "s_0 = sample.start mod N", "0 or any value >= N means N", "ties to the SMALLEST VISIT POSITION", "s <- (s + V) mod N",
                  "which is not kept", "failed nodes between the K-th and the", "first fit from a rotating start", "the one-worker reading",
                  "a = 50 - n / 125, raised to 5 when below 5", "raised to 100 when below 100", "(0 %, 1000) -> 420", "(0 %, 5000) -> 500",
                  "the context keeps no cursor between passes", "n_fit[i] = |C'|",
                  "TTL writes are defined as \"every node of the list offered\"", "upstream under sampling calls Filter on the visited"):
        assert words in HEADER, words
    assert HEADER.index("int bs_seq_run_scored_nominated(") < HEADER.index("F. (rule F.)") < HEADER.index("int bs_seq_run_scored_sampled("), \
        "the section sits behind bs_seq_run_scored_nominated"
    assert HEADER.index("D9. (recalled upstream") < HEADER.index("F. (rule F.)") < HEADER.index("Library rule F1:")


def test_null_context_is_refused_and_abi_version_stays():
    lib = capi.load_library()
    assert lib.bs_abi_version() == 7 and re.search(r"#define\s+BS_ABI_VERSION\s+7u", HEADER)
    o, w, s = capi.SeqOut(), capi.SeqScore(1, 0, 1), capi.SeqSample(1, 0)
    assert lib.bs_seq_run_scored_sampled(None, 1, C.byref(w), C.byref(s), C.byref(o)) == -1
    assert lib.bs_seq_run_scored_nominated_sampled(None, 1, 0, None, None, C.byref(w), C.byref(s), C.byref(o)) == -1
    assert lib.bs_seq_run_scored_sampled_flat(None, 1, 1, 0, 1, 1, 0, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.bs_seq_run_scored_nominated_sampled_flat(None, 1, 0, None, None, 1, 0, 1, 1, 0, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.bs_seq_sample_read(None, 0, None, None, None) == -1
    assert lib.bs_seq_sample_size(5000, 0) == 500, "pure arithmetic: no context"
