"""CPU: the model of bs_bound_apply (tests/bound_apply_ref.py) against sorting from scratch, against the device's merge rule restated
in Python, and against the hand known answers of tests/golden/bound_apply_hand_kats.json; and the built library exports the new entry
points, each answering a NULL context with BS_ERR_INVALID."""
import ctypes
import importlib

import numpy as np
import pytest

import bound_apply_ref as ba

bsa = importlib.import_module("batch-scheduler_amd")
soa, synth = bsa.soa, bsa.synth


def _sorted_from_scratch(t: ba.Table):
    """plain Python: every live entry as a tuple, sorted by (node, -priority, start, id)"""
    rows = [(int(t.node[i]), -int(t.priority[i]), int(t.start_ns[i]), int(t.id[i])) for i in range(t.count)]
    rows.sort()
    return [r[3] for r in rows], [r[0] for r in rows]


def _delta(rng, t: ba.Table, n_remove: int, n_insert: int, L: int, levels):
    rem = rng.permutation(t.id)[: min(n_remove, t.count)]
    ins = soa.Bound.empty(n_insert, L)
    ins.node[:] = rng.integers(0, t.n, n_insert)
    ins.priority[:] = rng.choice(levels, n_insert)
    ins.start_ns[:] = rng.integers(0, 4, n_insert) * 1_000_000_000
    ins.req[0] = rng.integers(1, 9, n_insert) * 100
    return rem, ins


@pytest.mark.parametrize("S,n,per", [(0, 1, (0, 40)), (1, 7, (0, 9)), (4, 40, (0, 5))])
def test_model_equals_sorting_from_scratch_and_the_merge_rule(S, n, per):
    bound, _ = synth.make_bound(77 + n, n, 4, per, S)
    levels = np.unique(bound.priority) if bound.b else np.array([0, 5], np.int32)
    rng = np.random.default_rng(4242 + n)
    t = ba.Table(bound, S, n)
    for step in range(12):
        before = t.table()
        rem, ins = _delta(rng, t, int(rng.integers(0, 6)), int(rng.integers(0, 8)), 4 + S, levels)
        first = t.apply(rem, ins, rng.integers(0, 2, ins.b))
        assert first + ins.b == t.ids
        got = t.table()
        ids, nodes = _sorted_from_scratch(t)
        assert got["id"].tolist() == ids and got["node"].tolist() == nodes, f"step {step}"
        # the device's rule, node by node: survivors in their old order, the inserts sorted by (importance, id)
        for k in range(n):
            old = before["id"][before["node"] == k]
            surv = [int(i) for i in old if i not in set(rem.tolist())]
            new = [int(first + i) for i in np.lexsort((np.arange(ins.b), ins.start_ns, -ins.priority.astype(np.int64))) if ins.node[i] == k]
            at = {int(i): j for j, i in enumerate(t.id)}
            key = lambda i: (int(t.priority[at[i]]), int(t.start_ns[at[i]]))      # noqa: E731
            ps, pi = ba.merge_positions([key(i)[0] for i in surv], [key(i)[1] for i in surv], [key(i)[0] for i in new], [key(i)[1] for i in new])
            merged = [None] * (len(surv) + len(new))
            for i, p in zip(surv + new, ps + pi):
                assert merged[p] is None, "two entries at one position"
                merged[p] = i
            assert merged == got["id"][got["node"] == k].tolist(), f"step {step} node {k}"
        # the equivalent table, loaded from scratch, is the same table through the id map
        eq, keep, bits = t.equivalent()
        t2 = ba.Table(eq, S, n, bits).table()
        assert np.array_equal(keep[t2["id"]], got["id"]) and np.all(np.diff(keep) > 0)
        for f in ("node",) + ba.COLUMNS:
            assert np.array_equal(t2[f], got[f]), f


def test_hand_known_answers():
    kats = ba.hand_kats()
    assert {k["name"] for k in kats} >= {"tie_with_a_survivor", "ties_among_inserts", "front_middle_end", "remove_and_insert_on_one_node",
                                         "a_node_emptied", "a_node_filled_from_empty"}
    for sc in kats:
        t = ba.Table(ba.kat_bound(sc["bound"]), 0, sc["n"])
        for i, st in enumerate(sc["steps"]):
            first = t.apply(st["remove"], ba.kat_bound(st["insert"]))
            got = t.table()
            assert first == st["first_id"], (sc["name"], i)
            assert got["id"].tolist() == st["id"] and got["node"].tolist() == st["node"], (sc["name"], i, got["id"].tolist())


def test_model_errors_change_nothing():
    bound, _ = synth.make_bound(5, 3, 0, 4, 0)
    t = ba.Table(bound, 0, 3)
    t.apply([2], None)
    before = t.table()
    one = ba.kat_bound({"node": [0], "priority": [1], "start_ns": [1]})
    bad_node = ba.kat_bound({"node": [3], "priority": [1], "start_ns": [1]})
    bad_group = ba.kat_bound({"node": [0], "priority": [1], "start_ns": [1]})
    bad_group.group[0] = -3
    for rem, ins in (([99], None), ([2], None), ([1, 1], None), ([], bad_node), ([], bad_group), ([2], one)):
        with pytest.raises(ba.ApplyError) as e:
            t.apply(rem, ins)
        assert e.value.status == -1
        after = t.table()
        assert all(np.array_equal(before[f], after[f]) for f in before) and t.ids == bound.b
    many = soa.Bound.empty(ba.MAX_PER_NODE - 4, 4)
    many.node[:] = 1
    assert t.apply([], many) == bound.b                                          # exactly the limit
    with pytest.raises(ba.ApplyError) as e:
        t.apply([], ba.kat_bound({"node": [1], "priority": [1], "start_ns": [1]}))
    assert e.value.status == -5


def test_library_exports_the_entry_points_and_refuses_a_null_context():
    lib = ctypes.CDLL(bsa.build.build())
    for name in ("bs_bound_apply", "bs_bound_apply_flat", "bs_bound_ids", "bs_bound_dump"):
        assert hasattr(lib, name), f"libbsched.so does not export {name}"
        assert name in bsa.capi.ABI_SYMBOLS
    d = soa.BoundDeltaStruct()
    v = ctypes.c_uint32()
    assert lib.bs_bound_apply(None, ctypes.byref(d), None) == -1
    assert lib.bs_bound_apply_flat(None, 0, None, 0, None, None, None, None, None, None, None, None) == -1
    assert lib.bs_bound_ids(None, ctypes.byref(v)) == -1
    assert lib.bs_bound_dump(None, None, None, None, None, None, None) == -1
    assert lib.bs_abi_version() == 7
