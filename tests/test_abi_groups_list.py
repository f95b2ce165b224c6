"""The C ABI of bs_groups_list_apply (include/bsched.h): the two declarations and their argument lists, the two structs, capi.ABI_SYMBOLS and
the binding, the exported symbols, a NULL context refused, and the ABI version (the call is additive: it stays 7).  No GPU: nothing here
creates a context."""
import ctypes as C
import importlib
import os
import re

bsa = importlib.import_module("batch-scheduler_amd")
capi = bsa.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bsched.h")).read()
ARGS = ["bs_ctx* ctx", "const bs_groups_list_delta* delta", "bs_groups_list_out* out"]
FLAT = ["bs_ctx* ctx", "uint32_t n_remove", "const uint32_t* remove", "uint32_t n_update", "const uint32_t* update", "uint32_t rows_g",
        "const uint32_t* min_member", "const uint32_t* status_scheduled", "const uint32_t* matched", "const uint8_t* flags", "const uint32_t* cls",
        "const int64_t* min_resources", "const uint32_t* min_resources_present", "const uint64_t* occupied_by", "uint32_t n_append",
        "uint32_t wait_cap", "uint32_t* wait_id", "uint32_t* wait_node", "int32_t* wait_group", "uint32_t* counts_out"]


def declared(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, re.S)
    assert m, f"{name} is not declared in include/bsched.h"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [re.sub(r"\s+", " ", a).strip() for a in args.split(",")], m


def test_the_declarations():
    args, m = declared("bs_groups_list_apply")
    assert args == ARGS
    assert declared("bs_groups_list_apply_flat")[0] == FLAT
    assert re.search(r"#define\s+BS_ABI_VERSION\s+7u", HEADER)
    assert HEADER.index("int bs_wait_nodes_apply(") < m.start() < HEADER.index("gang-aware preemption: the victim search"), "behind the wait table's blocks"


def fields(name):
    m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", HEADER, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ = decl.split()[0] if not decl.startswith("const") else "const " + decl.split()[1]
            out += [(typ, re.sub(r"[\s*]", "", x)) for x in decl[len(typ):].split(",")]
    return out


def test_the_structs_and_their_ctypes_mirrors():
    d = [n for _, n in fields("bs_groups_list_delta")]
    assert d == ["n_remove", "remove", "n_update", "update", "rows", "n_append"] == [n for n, _ in capi.GroupsListDelta._fields_]
    o = [n for _, n in fields("bs_groups_list_out")]
    assert sorted(o) == sorted(n for n, _ in capi.GroupsListOut._fields_)
    assert o == ["g_new", "n_pods_missing", "n_bound_missing", "n_wait_dropped", "wait_cap", "wait_id", "wait_node", "wait_group"] == \
        [n for n, _ in capi.GroupsListOut._fields_]
    # two uint32 + pointer pairs, the soa struct, one uint32: the layout a C compiler gives the header's struct on LP64
    assert capi.GroupsListDelta.remove.offset == 8 and capi.GroupsListDelta.rows.offset == 32 and capi.GroupsListDelta.rows.size == C.sizeof(bsa.soa.GroupsStruct)
    assert capi.GroupsListOut.wait_cap.offset == 16 and capi.GroupsListOut.wait_id.offset == 24 and C.sizeof(capi.GroupsListOut) == 48


def test_the_header_states_the_semantics_and_points_to_the_call():
    block = HEADER[HEADER.index("group-list surgery: PodGroups enter and leave the cache"):HEADER.index("typedef struct bs_groups_list_delta")]
    for cite in ("controller.go:194-196", ":226", ":143", ":167", ":305", "core.go:223-225", ":275-278"):
        assert cite in block, cite
    validity = HEADER.split("the table remembers the node count and the group count it was created for")[1][:900]
    assert "bs_wait_nodes_apply" in validity and "bs_groups_list_apply" in validity
    cycle = HEADER[HEADER.index("bs_pods_apply -> bs_seq_run -> bs_wait_release(released_group)"):][:700]
    assert "bs_groups_list_apply" in cycle and "parks first" in cycle
    assert "bs_groups_list_apply" in HEADER[HEADER.index("int bs_groups_read("):HEADER.index("typedef struct bs_group_delta")]


def test_the_symbols_are_listed_bound_and_exported():
    lib = capi.load_library()
    for name, n in (("bs_groups_list_apply", len(ARGS)), ("bs_groups_list_apply_flat", len(FLAT))):
        assert name in capi.ABI_SYMBOLS
        assert hasattr(lib, name), f"libbsched.so does not export {name}"
        assert len(getattr(lib, name).argtypes) == n
    assert hasattr(bsa.Context, "groups_list_apply")


def test_a_null_context_is_refused_and_the_abi_version_stays():
    lib = capi.load_library()
    assert lib.bs_abi_version() == 7
    d, o, cnt = capi.GroupsListDelta(), capi.GroupsListOut(), (C.c_uint32 * 4)()
    assert lib.bs_groups_list_apply(None, C.byref(d), C.byref(o)) == -1
    assert lib.bs_groups_list_apply_flat(None, 0, None, 0, None, 0, None, None, None, None, None, None, None, None, 0, 0, None, None, None, cnt) == -1
