"""PodDisruptionBudgets to bs_bound_pdb_set's bit array: the string work of upstream's filterPodsWithPDBViolation (k8s v1.17.5,
generic_scheduler.go), kept on the host.  The device only sees one bit per bound pod.

Recalled upstream semantics (the source is not vendored; include/bsched.h D1 states the rule the device relies on):
  M1. a PDB is looked at for a pod only when pdb.Namespace == pod.Namespace;
  M2. a pod without labels matches no PDB;
  M3. the selector goes through metav1.LabelSelectorAsSelector; a selector that does not parse skips the PDB;
  M4. a nil selector and an empty selector (no matchLabels, no matchExpressions) match nothing;
  M5. a matching PDB with Status.PodDisruptionsAllowed <= 0 makes the pod violating; one such PDB is enough.  Nothing is counted down.
LabelSelectorAsSelector: every matchLabels pair is an equality requirement; matchExpressions take In / NotIn (values required),
Exists / DoesNotExist (no values allowed); any other operator, a bad key or a bad value is an error.  NotIn and DoesNotExist match a
pod that lacks the key.

Records are plain dicts:
  pdb  {"namespace": str, "selector": None | {"matchLabels": {k: v}, "matchExpressions": [{"key", "operator", "values"}]},
        "disruptions_allowed": int}
  pod  {"namespace": str, "labels": {k: v} | None}
"""
from __future__ import annotations

import numpy as np

from .fitspec import label_key_ok, label_value_ok

_SET_OPS = ("In", "NotIn")
_KEY_OPS = ("Exists", "DoesNotExist")


def parse_selector(selector):
    """LabelSelectorAsSelector: a list of (key, operator, values) requirements; [] for an empty selector (M4: matches nothing here);
    None for a nil selector; raises ValueError for one that does not parse."""
    if selector is None:
        return None
    reqs = []
    for k, v in sorted((selector.get("matchLabels") or {}).items()):
        if not isinstance(k, str) or not isinstance(v, str) or not label_key_ok(k) or not label_value_ok(v):
            raise ValueError(f"matchLabels {k!r}: {v!r}")
        reqs.append((k, "In", (v,)))
    for e in selector.get("matchExpressions") or []:
        key, op, values = e.get("key"), e.get("operator"), tuple(e.get("values") or ())
        if not isinstance(key, str) or not label_key_ok(key):
            raise ValueError(f"matchExpressions key {key!r}")
        if op in _SET_OPS:
            if not values:
                raise ValueError(f"{op} needs values")
        elif op in _KEY_OPS:
            if values:
                raise ValueError(f"{op} takes no values")
        else:
            raise ValueError(f"operator {op!r}")
        if any(not isinstance(v, str) or not label_value_ok(v) for v in values):
            raise ValueError(f"matchExpressions values of {key!r}")
        reqs.append((key, op, values))
    return reqs


def selector_matches(reqs, labels: dict) -> bool:
    """labels.Selector.Matches for the parsed requirements (all must hold)"""
    for key, op, values in reqs:
        has = key in labels
        if op == "In":
            ok = has and labels[key] in values
        elif op == "NotIn":
            ok = not has or labels[key] not in values
        elif op == "Exists":
            ok = has
        else:
            ok = not has
        if not ok:
            return False
    return True


def violating_bits(pdbs, bound_pods) -> np.ndarray:
    """violating[b] for Context.bound_pdb_set: bound_pods[i] is the record of bound-pod id i (the numbering of the bound table load)."""
    parsed = []
    for pdb in pdbs:
        if int(pdb.get("disruptions_allowed", 0)) > 0:
            continue                                     # M5: only exhausted budgets can make a pod violating
        try:
            reqs = parse_selector(pdb.get("selector"))
        except ValueError:
            continue                                     # M3
        if not reqs:
            continue                                     # M4
        parsed.append((pdb.get("namespace", ""), reqs))
    out = np.zeros(len(bound_pods), np.uint8)
    for i, pod in enumerate(bound_pods):
        labels = pod.get("labels")
        if not labels:
            continue                                     # M2
        ns = pod.get("namespace", "")
        out[i] = any(pns == ns and selector_matches(reqs, labels) for pns, reqs in parsed)   # M1
    return out


def matching_members(pdbs, bound_pods):
    """(member_off, member) for Context.pdb_load / pdb_members_append: the PDBs that select each bound pod, by M1-M4 alone —
    disruptions_allowed is not looked at, that is the device's half (M5 over Context.pdb_allowed_apply's vector).  member_off is
    uint32 [len(bound_pods) + 1] from 0, member holds PDB indices, ascending within a pod.  A PDB whose selector is unparsable, nil
    or empty keeps its index and matches nobody."""
    parsed = []
    for pdb in pdbs:
        try:
            reqs = parse_selector(pdb.get("selector"))
        except ValueError:
            reqs = None                                  # M3
        parsed.append((pdb.get("namespace", ""), reqs or None))   # M4
    off = np.zeros(len(bound_pods) + 1, np.uint32)
    member = []
    for i, pod in enumerate(bound_pods):
        labels = pod.get("labels")
        if labels:                                       # M2
            ns = pod.get("namespace", "")
            member += [m for m, (pns, reqs) in enumerate(parsed) if reqs is not None and pns == ns and selector_matches(reqs, labels)]   # M1
        off[i + 1] = len(member)
    return off, np.asarray(member, np.uint32)


def allowed_vector(pdbs) -> np.ndarray:
    """allowed[n_pdb] for Context.pdb_load: every PDB's Status.PodDisruptionsAllowed (absent: 0, as violating_bits reads it)"""
    return np.asarray([int(pdb.get("disruptions_allowed", 0)) for pdb in pdbs], np.int32).reshape(-1)
