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
