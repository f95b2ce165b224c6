"""Array model of bs_groups_list_apply, written from the header text of include/bsched.h alone ("group-list surgery"): the new group list, the
remap of the three group columns (queue, bound table, wait table) and the wait rows that are dropped.  numpy only; the group list is any object
with the eight columns of bs_groups_soa as attributes (soa.Groups) — `make` builds the result with the same type."""
import numpy as np

COLUMNS = ("min_member", "status_scheduled", "matched", "flags", "cls", "min_resources", "min_resources_present", "occupied_by")
MISSING, NOT_GROUPED = -2, -1
OK, E_NULL, E_ROWS, E_RANGE, E_ORDER = 0, 1, 2, 3, 4      # csrc/bs_groups_list_check.hpp
INT_MAX = 2 ** 31 - 1


def check(g, remove, update, rows_g, n_append, rows_null=False, wait_cap=0, wait_null=False, remove_null=False, update_null=False):
    """the header's BS_ERR_INVALID cases in the order the library looks for them: NULL arrays, the row count, the remove list, the update list;
    inside a list entry by entry, the range before the order"""
    if (len(remove) and remove_null) or (len(update) and update_null) or (rows_g and rows_null) or (wait_cap and wait_null):
        return E_NULL
    if rows_g != len(update) + n_append:
        return E_ROWS
    for lst in (remove, update):
        for i, x in enumerate(lst):
            if x >= g:
                return E_RANGE
            if i and x <= lst[i - 1]:
                return E_ORDER
    return OK


def index_map(g, remove):
    """[g] int32: old group i -> i minus the removed indices below it, -1 for a removed group"""
    gone = np.zeros(g, bool)
    gone[np.asarray(remove, np.int64)] = True
    new = (np.arange(g) - np.cumsum(gone) + gone).astype(np.int32)          # (cumsum counts i itself when it is removed)
    new[gone] = -1
    return new


def remap(col, imap):
    """a group column under the map: values in 0 .. g_old - 1 follow it, a removed group becomes MISSING, everything else stays.
    -> (column, entries that became MISSING)"""
    col = np.asarray(col, np.int32).copy()
    inside = (col >= 0) & (col < imap.size)
    new = imap[col[inside]]
    col[inside] = np.where(new < 0, MISSING, new)
    return col, int((new < 0).sum())


def new_groups(groups, remove, update, rows, make=None):
    """the new list: survivors in their old order (an updated one takes its row of `rows`, an updated AND removed one is removed), then the
    appended rows"""
    make = make or type(groups)
    g, remove, update = groups.min_member.shape[0], list(remove), list(update)
    keep = np.array([i for i in range(g) if i not in set(remove)], np.int64)
    out = []
    for name in COLUMNS:
        old, new = np.asarray(getattr(groups, name)), np.asarray(getattr(rows, name))
        cur = old.copy()
        for u, i in enumerate(update):
            cur[..., i] = new[..., u]
        out.append(np.concatenate([cur[..., keep], new[..., len(update):]], axis=-1))
    return make(*out)


def max_group(m, g, remove):
    """the largest group index a table is held to name, after the remap: an upper bound that follows the map"""
    if m < 0 or m >= g:
        return m
    return m - sum(1 for x in remove if x <= m)


def list_apply(groups, remove, update, rows, pod_group=None, bound_group=None, wait=None, leader=-1, make=None):
    """everything the call changes.  wait: dict(id, node, group, req [L][w], req_present) in table order, or None.
    -> dict(groups, g_new, pod_group, n_pods_missing, bound_group, n_bound_missing, wait, dropped=(id, node, OLD group), leader)"""
    g = groups.min_member.shape[0]
    imap = index_map(g, remove)
    out = dict(groups=new_groups(groups, remove, update, rows, make), map=imap)
    out["g_new"] = out["groups"].min_member.shape[0]
    out["pod_group"], out["n_pods_missing"] = remap(pod_group, imap) if pod_group is not None else (None, 0)
    out["bound_group"], out["n_bound_missing"] = remap(bound_group, imap) if bound_group is not None else (None, 0)
    out["leader"] = int(imap[leader]) if 0 <= leader < g else leader
    if wait is not None:
        grp = np.asarray(wait["group"], np.int32)
        gone = (grp >= 0) & (grp < g)
        gone[gone] = imap[grp[gone]] < 0
        keep = ~gone
        out["dropped"] = (np.asarray(wait["id"])[gone].copy(), np.asarray(wait["node"])[gone].copy(), grp[gone].copy())
        out["wait"] = dict(id=np.asarray(wait["id"])[keep].copy(), node=np.asarray(wait["node"])[keep].copy(), group=remap(grp[keep], imap)[0],
                           req=np.asarray(wait["req"])[:, keep].copy(), req_present=np.asarray(wait["req_present"])[keep].copy())
    else:
        out["wait"], out["dropped"] = None, (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.int32))
    return out


# ---- a second statement, object by object: a list of group records and tables of records that POINT at them -------------------------------
def naive(group_rows, remove, update, new_rows, pod_group, bound_group, wait_rows):
    """group_rows: list of opaque records.  pod_group / bound_group: lists of indices or sentinels.  wait_rows: list of (id, node, group).
    Rebuilds the list by walking it, resolves every reference through object identity.  -> (rows, pod_group, bound_group, kept, dropped)"""
    cells = [[r] for r in group_rows]                                           # one mutable cell per group: identity survives the surgery
    for u, i in enumerate(update):
        cells[i][0] = new_rows[u]
    removed = set(remove)
    alive = [c for i, c in enumerate(cells) if i not in removed]
    alive += [[r] for r in new_rows[len(update):]]
    where = {id(c): k for k, c in enumerate(alive)}

    def follow(v):
        if v < 0 or v >= len(cells):
            return v
        return where.get(id(cells[v]), MISSING)
    kept, dropped = [], []
    for (i, n, gidx) in wait_rows:
        if 0 <= gidx < len(cells) and follow(gidx) == MISSING:
            dropped.append((i, n, gidx))
        else:
            kept.append((i, n, follow(gidx)))
    return [c[0] for c in alive], [follow(v) for v in pod_group], [follow(v) for v in bound_group], kept, dropped


def random_delta(rng, g, rows_for, max_append=4):
    """a valid random delta on g groups: (remove, update, rows, n_append); rows_for(n) makes n new rows.  Most deltas are a few events; one in
    ten removes every group, one in five removes many"""
    u = rng.random()
    k = g if u < 0.1 else int(rng.integers(0, g + 1)) if u < 0.3 else int(rng.integers(0, min(g, 3) + 1))
    remove = sorted(rng.choice(g, k, replace=False).tolist()) if k else []
    k = int(rng.integers(0, min(g, 3) + 1)) if rng.random() < 0.5 else 0
    update = sorted(rng.choice(g, k, replace=False).tolist()) if k else []
    n_append = int(rng.integers(0, max_append + 1))
    return remove, update, rows_for(len(update) + n_append), n_append
