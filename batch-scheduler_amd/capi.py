"""ctypes binding of the C ABI (include/bsched.h) implemented by libbsched.so (HIP, gfx950).

This is what a host language does at the boundary: hand flat SoA buffers in, get decision arrays
out.  No torch types cross it.  There is deliberately NO fallback: a missing library, a missing
GPU or a failing HIP call raises BsError.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import fitspec, soa

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.environ.get("BS_LIB_DIR") or HERE, "libbsched.so")      # (BS_LIB_DIR: see build.py)

KERNEL_COUNT = 8
KERNEL_PREPASS, KERNEL_LEADER, KERNEL_QUERY, KERNEL_TABLES, KERNEL_SCAN, KERNEL_RESOLVE, KERNEL_FILTER, KERNEL_TALLY = range(8)

# every symbol include/bsched.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "bs_abi_version", "bs_strerror", "bs_last_error", "bs_create", "bs_destroy",
    "bs_nodes_load", "bs_fit_load", "bs_fit_build", "bs_fit_read", "bs_groups_load", "bs_groups_read", "bs_groups_apply", "bs_pods_map", "bs_pods_load",
    "bs_pods_apply", "bs_pods_count", "bs_pods_read", "bs_pods_apply_stats", "bs_filter_deny_stats", "bs_speculation_stats",
    "bs_nodes_apply", "bs_nodes_count", "bs_nodes_assume",
    "bs_cluster_fits", "bs_node_left", "bs_scan_prefix", "bs_cluster_total", "bs_filter_one", "bs_find_max_pg",
    "bs_batch_run", "bs_batch_sync", "bs_batch_read", "bs_batch_map", "bs_filter_rows_count", "bs_queue_order_load", "bs_queue_sort",
    "bs_shard_set", "bs_reduce_external", "bs_group_admit_devptr", "bs_group_admit_bind", "bs_stream", "bs_comm_unique_id", "bs_comm_init", "bs_batch_finish",
    "bs_timing_reset", "bs_timing_get", "bs_kernel_name", "bs_batch_stats_get",
    "bs_seq_run", "bs_nodes_read", "bs_first_reach_hint",
    "bs_nodes_load_flat", "bs_groups_load_flat", "bs_groups_read_flat", "bs_pods_load_flat", "bs_pods_apply_flat", "bs_pods_read_flat",
    "bs_batch_read_flat", "bs_seq_run_flat", "bs_fit_build_flat",
    "bs_bound_load", "bs_bound_count", "bs_preempt_run", "bs_bound_load_flat", "bs_preempt_run_flat",
    "bs_preempt_commit", "bs_bound_read", "bs_preempt_commit_flat",
    "bs_bound_pdb_set", "bs_preempt_pdb_read",
    "bs_bound_apply", "bs_bound_apply_flat", "bs_bound_ids", "bs_bound_dump",
    "bs_bound_nodes_apply",
    "bs_bound_apply_ex", "bs_bound_apply_ex_flat",
    "bs_pdb_load", "bs_pdb_members_append", "bs_pdb_allowed_apply", "bs_pdb_read",
    "bs_preempt_commit_gang", "bs_preempt_commit_gang_flat", "bs_preempt_gang_read",
    "bs_seq_expire", "bs_seq_expire_flat", "bs_seq_waiting_read",
    "bs_wait_load", "bs_wait_count", "bs_wait_ids", "bs_wait_read", "bs_wait_park", "bs_wait_release", "bs_wait_expire", "bs_wait_forget",
    "bs_wait_nodes_apply",
    "bs_groups_list_apply", "bs_groups_list_apply_flat",
    "bs_bound_bind",
    "bs_nominated_load", "bs_nominated_count", "bs_nominated_ids", "bs_nominated_read", "bs_nominated_apply", "bs_preempt_nominated_read",
    "bs_nominated_nodes_apply",
    "bs_preempt_cleared_read",
    "bs_seq_run_nominated", "bs_seq_run_nominated_flat", "bs_seq_nominated_read",
    "bs_seq_run_scored", "bs_seq_run_scored_flat", "bs_seq_score_read",
    "bs_seq_run_scored_nominated", "bs_seq_run_scored_nominated_flat",
    "bs_seq_sample_size", "bs_seq_run_scored_sampled", "bs_seq_run_scored_sampled_flat", "bs_seq_run_scored_nominated_sampled",
    "bs_seq_run_scored_nominated_sampled_flat", "bs_seq_sample_read",
]

SEQ_EXPIRE_DENY, SEQ_EXPIRE_ALL = 1, 2    # bs_seq_expire flags
WAIT_MAX = 1 << 24                        # BS_WAIT_MAX: rows and ids of the wait table
NOM_MAX = 1 << 16                         # BS_NOM_MAX: live rows of the nominated-pod table (its id space goes up to 2^24)
NOM_NONE = 0xFFFFFFFF                     # bs_preempt_nominated_read: the preemptor got no row
SCORE_WEIGHT_MAX = 65536                  # BS_SCORE_WEIGHT_MAX: each weight of bs_seq_score

BS_BOUND_NODES = soa.BS_BOUND_NODES     # bs_bound_apply_ex: the delta also moves the node requests

# bsh_phase codes (include/bsched_host.h) of the phases whose gangs PreemptRemovePod protects: Running and Scheduled (core.go:235-238)
PROTECTED_PHASES = (2, 5)


def group_protected(phases) -> np.ndarray:
    """bs_preempt_run's group_protected[g] from each group's bsh_phase code: 1 where the phase is Scheduled or Running."""
    ph = np.asarray(phases, dtype=np.int64).reshape(-1)
    return np.isin(ph, PROTECTED_PHASES).astype(np.uint8)


def gang_order(pod_group, priority) -> np.ndarray:
    """A permutation of the caller's preemptor list for bs_preempt_commit_gang: priority descending (stable), then by first appearance
    of the group within the priority, members in the caller's order; preemptors without a group index >= 0 count as groups of their
    own.  Every gang of equal-priority members becomes one run of slots."""
    grp = np.asarray(pod_group, np.int64).reshape(-1)
    pri = np.asarray(priority, np.int64).reshape(-1)
    assert grp.shape == pri.shape
    first: dict = {}
    rank = np.zeros(grp.shape[0], np.int64)
    for i in range(grp.shape[0]):
        key = (int(pri[i]), int(grp[i])) if grp[i] >= 0 else (int(pri[i]), -1 - i)
        rank[i] = first.setdefault(key, i)
    return np.lexsort((np.arange(grp.shape[0]), rank, -pri)).astype(np.int64)


def gang_need(groups, waiting=None) -> np.ndarray:
    """bs_preempt_commit_gang's gang_need[g] from the loaded groups: MinMember minus Status.Scheduled minus the members already waiting
    at Permit (waiting[g], default 0), never below 0: how many more members must get a node for the gang to pass its quorum."""
    mm = np.asarray(groups.min_member, np.int64).reshape(-1)
    w = np.zeros_like(mm) if waiting is None else np.asarray(waiting, np.int64).reshape(-1)
    assert w.shape == mm.shape
    return np.clip(mm - np.asarray(groups.status_scheduled, np.int64).reshape(-1) - w, 0, None).astype(np.uint32)


class BsError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: status {status}" + (f" ({detail})" if detail else ""))


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("scalar_lanes", C.c_uint32),
                ("eph_gate", C.c_uint32), ("enable_timing", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class NodeDelta(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32),
                ("allocatable", C.c_int64 * soa.MAX_LANES), ("requested", C.c_int64 * soa.MAX_LANES),
                ("allocatable_present", C.c_uint32), ("requested_present", C.c_uint32), ("flags", C.c_uint32),
                ("fit_default", C.c_uint32), ("n_fit_exceptions", C.c_uint32), ("fit_exceptions", C.c_uint32 * 8)]


class NodeRequest(C.Structure):
    _fields_ = [("index", C.c_uint32), ("requested_present", C.c_uint32), ("requested", C.c_int64 * soa.MAX_LANES)]


DELTA_UPDATE, DELTA_APPEND, DELTA_REMOVE = 0, 1, 2


class Timing(C.Structure):
    _fields_ = [("total_ms", C.c_double * KERNEL_COUNT), ("launches", C.c_uint64 * KERNEL_COUNT)]


class BatchStats(C.Structure):
    _fields_ = [("scan_queries", C.c_uint64), ("scan_rows_executed", C.c_uint64), ("scan_evals_executed", C.c_uint64),
                ("tables_built", C.c_uint64), ("logical_evals", C.c_uint64), ("filter_evals", C.c_uint64),
                ("filter_distinct", C.c_uint64), ("filter_evals_executed", C.c_uint64),
                ("scan_queries_logical", C.c_uint64), ("class_mode", C.c_uint64), ("fast_path", C.c_uint64), ("launches", C.c_uint64),
                ("chain", C.c_uint64), ("filter_lane_blocks", C.c_uint64), ("filter_tile_blocks", C.c_uint64)]


class SeqOut(C.Structure):
    """bs_seq_out"""
    _fields_ = [("pf_code", C.POINTER(C.c_uint8)), ("pf_first_k", C.POINTER(C.c_uint32)), ("pf_leader", C.POINTER(C.c_int32)),
                ("pod_node", C.POINTER(C.c_int32)), ("cap", C.c_uint32), ("released_group", C.POINTER(C.c_uint32)),
                ("released_pods", C.POINTER(C.c_uint32)), ("first_ns", C.POINTER(C.c_int64)), ("ready_ns", C.POINTER(C.c_int64)),
                ("n_released", C.c_uint32), ("total_ns", C.c_int64), ("node_picks", C.c_uint64), ("node_scans", C.c_uint64),
                ("scan_rounds", C.c_uint64), ("pick_rounds", C.c_uint64), ("leader_folds", C.c_uint64), ("table_builds", C.c_uint64),
                ("last_permitted", C.POINTER(C.c_uint8))]


class SeqScore(C.Structure):
    """bs_seq_score: the weights of rule P (each at most SCORE_WEIGHT_MAX)"""
    _fields_ = [("w_least", C.c_uint32), ("w_most", C.c_uint32), ("w_balanced", C.c_uint32)]


class SeqSample(C.Structure):
    """bs_seq_sample: rule F's K (0 or >= N: every candidate) and the cursor the pass starts at (taken mod N)"""
    _fields_ = [("num_to_find", C.c_uint32), ("start", C.c_uint32)]


class SeqExpireOut(C.Structure):
    """bs_seq_expire_out"""
    _fields_ = [("n_groups", C.c_uint32), ("n_pods", C.c_uint32), ("group_cap", C.c_uint32), ("group", C.POINTER(C.c_uint32)),
                ("group_pods", C.POINTER(C.c_uint32)), ("group_earlier", C.POINTER(C.c_uint32)), ("pod_cap", C.c_uint32),
                ("pod", C.POINTER(C.c_uint32)), ("node", C.POINTER(C.c_uint32))]


_lib = None


class GroupsListDelta(C.Structure):
    """bs_groups_list_delta"""
    _fields_ = [("n_remove", C.c_uint32), ("remove", C.POINTER(C.c_uint32)), ("n_update", C.c_uint32), ("update", C.POINTER(C.c_uint32)),
                ("rows", soa.GroupsStruct), ("n_append", C.c_uint32)]


class GroupsListOut(C.Structure):
    """bs_groups_list_out"""
    _fields_ = [("g_new", C.c_uint32), ("n_pods_missing", C.c_uint32), ("n_bound_missing", C.c_uint32), ("n_wait_dropped", C.c_uint32),
                ("wait_cap", C.c_uint32), ("wait_id", C.POINTER(C.c_uint32)), ("wait_node", C.POINTER(C.c_uint32)), ("wait_group", C.POINTER(C.c_int32))]


def load_library(path: str | None = None):
    """dlopen libbsched.so and declare prototypes.  Raises if the HIP library is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise BsError(-2, "load_library", f"{p} not built: run `python __graft_entry__.py build` (hipcc, gfx950)")
    L = C.CDLL(p)
    vp, u32, i32, u8 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint8
    P = C.POINTER
    L.bs_abi_version.restype = u32
    L.bs_strerror.restype = C.c_char_p
    L.bs_strerror.argtypes = [C.c_int]
    L.bs_last_error.restype = C.c_char_p
    L.bs_last_error.argtypes = [vp]
    L.bs_kernel_name.restype = C.c_char_p
    L.bs_kernel_name.argtypes = [u32]
    L.bs_create.argtypes = [P(Config), P(vp)]
    L.bs_destroy.argtypes = [vp]
    L.bs_nodes_load.argtypes = [vp, P(soa.NodesStruct)]
    L.bs_fit_load.argtypes = [vp, u32, P(u32)]
    L.bs_fit_build.argtypes = [vp, P(fitspec.NodeLabelsStruct), P(fitspec.FitTemplatesStruct)]
    L.bs_fit_read.argtypes = [vp, P(u32)]
    L.bs_groups_load.argtypes = [vp, P(soa.GroupsStruct)]
    L.bs_groups_read.argtypes = [vp, P(soa.GroupsStruct)]
    L.bs_groups_apply.argtypes = [vp, P(soa.GroupDelta), u32]
    L.bs_filter_rows_count.argtypes = [vp, P(u32)]
    L.bs_pods_load.argtypes = [vp, P(soa.PodsStruct)]
    L.bs_pods_map.argtypes = [vp, u32, P(soa.PodsStruct)]
    L.bs_pods_apply.argtypes = [vp, P(soa.PodsDeltaStruct)]
    L.bs_pods_count.argtypes = [vp, P(u32)]
    L.bs_pods_apply_stats.argtypes = [vp, P(C.c_uint64), P(C.c_uint64)]
    L.bs_filter_deny_stats.argtypes = [vp, P(C.c_uint64)]
    L.bs_speculation_stats.argtypes = [vp, P(C.c_uint64), P(C.c_uint64)]
    L.bs_pods_read.argtypes = [vp, P(soa.PodsOutStruct)]
    L.bs_queue_order_load.argtypes = [vp, u32, P(u32)]
    L.bs_queue_sort.argtypes = [vp, u32, P(i32), P(i32), P(C.c_int64), P(u32)]
    L.bs_nodes_apply.argtypes = [vp, P(NodeDelta), u32]
    L.bs_nodes_count.argtypes = [vp, P(u32)]
    L.bs_nodes_assume.argtypes = [vp, P(NodeRequest), u32]
    L.bs_cluster_fits.argtypes = [vp, u32, C.c_float, P(C.c_int64), u32, P(u8), P(u32)]
    L.bs_node_left.argtypes = [vp, u32, C.c_float, P(C.c_int64), P(u32)]
    L.bs_scan_prefix.argtypes = [vp, u32, C.c_float, P(C.c_int64), P(u32), P(u32), P(u32)]
    L.bs_cluster_total.argtypes = [vp, u32, P(C.c_int64), P(u32)]
    L.bs_filter_one.argtypes = [vp, i32, P(C.c_int64), u32, i32, u32, P(u8), P(u8)]
    L.bs_find_max_pg.argtypes = [vp, P(i32), P(u32), P(u8)]
    L.bs_batch_run.argtypes = [vp, u32]
    L.bs_batch_sync.argtypes = [vp]
    L.bs_batch_read.argtypes = [vp, P(soa.BatchOutStruct)]
    L.bs_batch_map.argtypes = [vp, P(soa.BatchViewStruct)]
    L.bs_shard_set.argtypes = [vp, u32, u32]
    L.bs_group_admit_devptr.argtypes = [vp, P(vp), P(u32)]
    L.bs_reduce_external.argtypes = [vp, u32]
    L.bs_first_reach_hint.argtypes = [vp, u32]
    L.bs_group_admit_bind.argtypes = [vp, vp]
    L.bs_stream.argtypes = [vp, P(vp)]
    L.bs_comm_unique_id.argtypes = [P(u8)]
    L.bs_comm_init.argtypes = [vp, P(u8), u32, u32]
    L.bs_batch_finish.argtypes = [vp]
    L.bs_timing_reset.argtypes = [vp]
    L.bs_timing_get.argtypes = [vp, P(Timing)]
    L.bs_batch_stats_get.argtypes = [vp, P(BatchStats)]
    L.bs_seq_run.argtypes = [vp, u32, P(SeqOut)]
    L.bs_nodes_read.argtypes = [vp, P(C.c_int64), P(u32)]
    L.bs_bound_load.argtypes = [vp, P(soa.BoundStruct)]
    L.bs_bound_count.argtypes = [vp, P(u32)]
    L.bs_preempt_run.argtypes = [vp, u32, u32, P(u32), P(i32), P(u8), u32, P(soa.PreemptOutStruct)]
    L.bs_bound_load_flat.argtypes = [vp, u32, P(u32), P(i32), P(C.c_int64), P(i32), P(C.c_int64), P(u32)]
    L.bs_preempt_run_flat.argtypes = [vp, u32, u32, P(u32), P(i32), P(u8), u32, P(i32), P(u32), P(u32), P(u32), P(i32), P(C.c_int64), P(C.c_int64)]
    L.bs_preempt_commit.argtypes = [vp, u32, u32, P(u32), P(i32), P(u8), u32, u32, P(soa.PreemptOutStruct)]
    L.bs_bound_read.argtypes = [vp, P(u32), P(u32)]
    L.bs_bound_pdb_set.argtypes = [vp, u32, P(u8)]
    L.bs_bound_apply.argtypes = [vp, P(soa.BoundDeltaStruct), P(u32)]
    L.bs_bound_apply_flat.argtypes = [vp, u32, P(u32), u32, P(u32), P(i32), P(C.c_int64), P(i32), P(C.c_int64), P(u32), P(u8), P(u32)]
    L.bs_bound_apply_ex.argtypes = [vp, P(soa.BoundDeltaStruct), u32, P(u32)]
    L.bs_bound_apply_ex_flat.argtypes = [vp, u32, u32, P(u32), u32, P(u32), P(i32), P(C.c_int64), P(i32), P(C.c_int64), P(u32), P(u8), P(u32)]
    L.bs_bound_ids.argtypes = [vp, P(u32)]
    L.bs_bound_nodes_apply.argtypes = [vp, u32, P(u32), P(u32), u32, P(u32), P(u32)]
    L.bs_bound_dump.argtypes = [vp, P(i32), P(C.c_int64), P(i32), P(C.c_int64), P(u32), P(u8)]
    L.bs_preempt_pdb_read.argtypes = [vp, u32, P(u32)]
    L.bs_pdb_load.argtypes = [vp, u32, P(i32), u32, P(u32), P(u32)]
    L.bs_pdb_members_append.argtypes = [vp, u32, u32, P(u32), P(u32)]
    L.bs_pdb_allowed_apply.argtypes = [vp, u32, P(u32), P(i32)]
    L.bs_pdb_read.argtypes = [vp, P(u32), P(u32), P(i32), P(u32)]
    L.bs_preempt_commit_flat.argtypes = [vp, u32, u32, P(u32), P(i32), P(u8), u32, u32, P(i32), P(u32), P(u32), P(u32), P(i32), P(C.c_int64),
                                         P(C.c_int64)]
    L.bs_preempt_commit_gang.argtypes = [vp, u32, u32, P(u32), P(i32), P(u8), P(u32), u32, u32, P(soa.PreemptOutStruct)]
    L.bs_preempt_commit_gang_flat.argtypes = [vp, u32, u32, P(u32), P(i32), P(u8), P(u32), u32, u32, P(i32), P(u32), P(u32), P(u32), P(i32),
                                              P(C.c_int64), P(C.c_int64)]
    L.bs_preempt_gang_read.argtypes = [vp, u32, P(u8), u32, P(u32)]
    L.bs_seq_expire.argtypes = [vp, u32, P(u32), u32, P(SeqExpireOut)]
    L.bs_seq_expire_flat.argtypes = [vp, u32, P(u32), u32, u32, P(u32), P(u32), P(u32), u32, P(u32), P(u32), P(u32)]
    L.bs_seq_waiting_read.argtypes = [vp, u32, P(i32)]
    L.bs_wait_load.argtypes = [vp, u32, P(u32), P(i32), P(C.c_int64), P(u32)]
    L.bs_wait_count.argtypes = [vp, P(u32)]
    L.bs_wait_ids.argtypes = [vp, P(u32)]
    L.bs_wait_read.argtypes = [vp, P(u32), P(u32), P(i32), P(C.c_int64), P(u32)]
    L.bs_wait_park.argtypes = [vp, u32, P(u32), P(u32), P(u32), P(u32)]
    L.bs_wait_release.argtypes = [vp, u32, P(u32), u32, P(u32), P(u32), P(u32), P(u32)]
    L.bs_wait_expire.argtypes = [vp, u32, P(u32), u32, u32, P(u32), P(u32), P(u32), P(u32), P(u32)]
    L.bs_wait_forget.argtypes = [vp, u32, P(u32), P(u32)]
    L.bs_wait_nodes_apply.argtypes = [vp, u32, P(u32), P(u32), u32, P(u32), P(u32), P(i32), P(u32)]
    L.bs_groups_list_apply.argtypes = [vp, P(GroupsListDelta), P(GroupsListOut)]
    L.bs_groups_list_apply_flat.argtypes = [vp, u32, P(u32), u32, P(u32), u32, P(u32), P(u32), P(u32), P(u8), P(u32), P(C.c_int64), P(u32), P(C.c_uint64),
                                            u32, u32, P(u32), P(u32), P(i32), P(u32)]
    L.bs_nominated_load.argtypes = [vp, u32, P(u32), P(i32), P(C.c_int64), P(u32)]
    L.bs_nominated_count.argtypes = [vp, P(u32)]
    L.bs_nominated_ids.argtypes = [vp, P(u32)]
    L.bs_nominated_read.argtypes = [vp, P(u32), P(u32), P(i32), P(C.c_int64), P(u32)]
    L.bs_nominated_apply.argtypes = [vp, u32, P(u32), u32, P(u32), P(u32), P(i32), P(u32)]
    L.bs_preempt_nominated_read.argtypes = [vp, u32, P(u32)]
    L.bs_preempt_cleared_read.argtypes = [vp, u32, P(u32), P(u32), P(i32), P(u32), P(u32)]
    L.bs_nominated_nodes_apply.argtypes = [vp, u32, P(u32), P(u32), u32, P(u32), P(u32), P(i32), P(u32)]
    L.bs_bound_bind.argtypes = [vp, u32, P(u32), u32, P(u32), P(i32), P(C.c_int64), P(u8), P(u32), P(u32)]
    L.bs_seq_run_nominated.argtypes = [vp, u32, u32, P(i32), P(u32), P(SeqOut)]
    L.bs_seq_run_nominated_flat.argtypes = [vp, u32, u32, P(i32), P(u32), P(u8), P(u32), P(i32), P(i32), u32, P(u32), P(u32), P(C.c_int64), P(C.c_int64),
                                            P(C.c_int64), P(u8)]
    L.bs_seq_nominated_read.argtypes = [vp, u32, P(u32), P(u32), P(u32), P(u32)]
    L.bs_seq_run_scored.argtypes = [vp, u32, P(SeqScore), P(SeqOut)]
    L.bs_seq_run_scored_flat.argtypes = [vp, u32, u32, u32, u32, P(u8), P(u32), P(i32), P(i32), u32, P(u32), P(u32), P(C.c_int64), P(C.c_int64),
                                         P(C.c_int64), P(u8)]
    L.bs_seq_score_read.argtypes = [vp, u32, P(u32), P(u32)]
    L.bs_seq_run_scored_nominated.argtypes = [vp, u32, u32, P(i32), P(u32), P(SeqScore), P(SeqOut)]
    L.bs_seq_run_scored_nominated_flat.argtypes = [vp, u32, u32, P(i32), P(u32), u32, u32, u32, P(u8), P(u32), P(i32), P(i32), u32, P(u32), P(u32), P(C.c_int64),
                                                   P(C.c_int64), P(C.c_int64), P(u8)]
    L.bs_seq_sample_size.argtypes = [u32, i32]
    L.bs_seq_sample_size.restype = u32
    L.bs_seq_run_scored_sampled.argtypes = [vp, u32, P(SeqScore), P(SeqSample), P(SeqOut)]
    L.bs_seq_run_scored_sampled_flat.argtypes = [vp, u32, u32, u32, u32, u32, u32, P(u8), P(u32), P(i32), P(i32), u32, P(u32), P(u32), P(C.c_int64),
                                                 P(C.c_int64), P(C.c_int64), P(u8)]
    L.bs_seq_run_scored_nominated_sampled.argtypes = [vp, u32, u32, P(i32), P(u32), P(SeqScore), P(SeqSample), P(SeqOut)]
    L.bs_seq_run_scored_nominated_sampled_flat.argtypes = [vp, u32, u32, P(i32), P(u32), u32, u32, u32, u32, u32, P(u8), P(u32), P(i32), P(i32), u32, P(u32),
                                                           P(u32), P(C.c_int64), P(C.c_int64), P(C.c_int64), P(u8)]
    L.bs_seq_sample_read.argtypes = [vp, u32, P(u32), P(u32), P(u32)]
    for name in ABI_SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int:
            fn.restype = C.c_int
    if path is None:
        _lib = L
    return L


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class Context:
    """One bs_ctx: a HIP device, its stream and the resident snapshot / group / pod state."""

    def __init__(self, scalar_lanes: int = 0, eph_gate: int = 1, device: int = 0, enable_timing: int = 0):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.S = scalar_lanes
        self.L = soa.FIXED_LANES + scalar_lanes
        cfg = Config(self._lib.bs_abi_version(), device, scalar_lanes, eph_gate, enable_timing)
        rc = self._lib.bs_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise BsError(rc, "bs_create", self._lib.bs_strerror(rc).decode())
        self.n = self.g = self.p = 0

    # -- plumbing
    def _chk(self, rc: int, where: str):
        if rc != 0:
            raise BsError(rc, where, self._lib.bs_strerror(rc).decode() + ": " + self._lib.bs_last_error(self._h).decode())

    def close(self):
        if self._h:
            self._lib.bs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- loads
    def load_nodes(self, nodes: soa.Nodes, fit: soa.FitMasks | None = None):
        assert nodes.lanes == self.L, f"context has {self.L} lanes, nodes have {nodes.lanes}"
        st = nodes.as_struct()
        self._chk(self._lib.bs_nodes_load(self._h, C.byref(st)), "bs_nodes_load")
        self.n = nodes.n
        if fit is not None:
            self.load_fit(fit)

    def load_fit(self, fit: soa.FitMasks):
        assert fit.n == self.n
        bits = np.ascontiguousarray(fit.bits, dtype=np.uint32)
        if bits.size == 0:
            bits = np.zeros((fit.n_classes, 1), np.uint32)
        self._chk(self._lib.bs_fit_load(self._h, fit.n_classes, _u32p(bits)), "bs_fit_load")
        self.n_classes = fit.n_classes

    def build_fit(self, node_labels: "fitspec.NodeLabels", templates: "fitspec.FitTemplates"):
        """checkFit (core.go:741-759) for every (class, node) on the device; replaces load_fit."""
        assert node_labels.n == self.n
        ns, ts = node_labels.as_struct(), templates.as_struct()
        self._chk(self._lib.bs_fit_build(self._h, C.byref(ns), C.byref(ts)), "bs_fit_build")
        self.n_classes = templates.c

    def read_fit(self) -> soa.FitMasks:
        words = (self.n + 31) // 32
        bits = np.zeros(self.n_classes * words + 1, np.uint32)        # +1: never hand out a NULL pointer
        self._chk(self._lib.bs_fit_read(self._h, _u32p(bits)), "bs_fit_read")
        return soa.FitMasks(bits[:-1].reshape(self.n_classes, words).copy(), self.n)

    def load_groups(self, groups: soa.Groups):
        assert groups.min_resources.shape[0] == self.L
        st = groups.as_struct()
        self._chk(self._lib.bs_groups_load(self._h, C.byref(st)), "bs_groups_load")
        self.g = groups.g

    def read_groups(self) -> soa.Groups:
        out = soa.Groups.empty(self.g, self.L)
        st = out.as_struct()
        self._chk(self._lib.bs_groups_read(self._h, C.byref(st)), "bs_groups_read")
        return out

    def groups_list_apply(self, remove=(), update=(), rows: "soa.Groups | None" = None, n_append: int | None = None, wait_cap: int | None = None,
                          flat: bool = False) -> dict:
        """bs_groups_list_apply: PodGroups enter and leave the cache.  remove / update: OLD group indices, strictly ascending; rows: the
        updated groups' new rows in `update` order, then the appended groups (n_append defaults to rows.g - len(update)).  The group list,
        the queue's group column, the bound table's and the wait table's follow in one call.  Returns the out struct as a dict: g_new,
        n_pods_missing, n_bound_missing, n_wait_dropped and the dropped wait rows wait_id, wait_node, wait_group (OLD group index; at most
        wait_cap rows, the default holds the whole table).  flat=True goes through bs_groups_list_apply_flat."""
        rv = np.ascontiguousarray(np.asarray(remove, np.uint32).reshape(-1))
        uv = np.ascontiguousarray(np.asarray(update, np.uint32).reshape(-1))
        rows = soa.Groups.empty(0, self.L) if rows is None else rows
        assert rows.min_resources.shape[0] == self.L
        n_append = rows.g - int(uv.size) if n_append is None else int(n_append)
        if wait_cap is None:
            w = C.c_uint32(0)
            wait_cap = int(w.value) if self._lib.bs_wait_count(self._h, C.byref(w)) == 0 else 0
        cap = int(wait_cap)
        wi, wn, wg = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.int32)
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rs = rows.as_struct()
        if flat:
            cnt = np.zeros(4, np.uint32)
            self._chk(self._lib.bs_groups_list_apply_flat(
                self._h, int(rv.size), _u32p(rv) if rv.size else None, int(uv.size), _u32p(uv) if uv.size else None, rs.g, rs.min_member, rs.status_scheduled,
                rs.matched, rs.flags, rs.cls, rs.min_resources, rs.min_resources_present, rs.occupied_by, n_append, cap, _u32p(wi) if cap else None,
                _u32p(wn) if cap else None, i32p(wg) if cap else None, _u32p(cnt)), "bs_groups_list_apply_flat")
            g_new, pm, bm, wd = (int(x) for x in cnt)
        else:
            d = GroupsListDelta(int(rv.size), _u32p(rv) if rv.size else None, int(uv.size), _u32p(uv) if uv.size else None, rs, n_append)
            o = GroupsListOut(0, 0, 0, 0, cap, _u32p(wi) if cap else None, _u32p(wn) if cap else None, i32p(wg) if cap else None)
            self._chk(self._lib.bs_groups_list_apply(self._h, C.byref(d), C.byref(o)), "bs_groups_list_apply")
            g_new, pm, bm, wd = int(o.g_new), int(o.n_pods_missing), int(o.n_bound_missing), int(o.n_wait_dropped)
        self.g = g_new
        k = min(wd, cap)
        return dict(g_new=g_new, n_pods_missing=pm, n_bound_missing=bm, n_wait_dropped=wd, wait_id=wi[:k].copy(), wait_node=wn[:k].copy(),
                    wait_group=wg[:k].copy())

    def apply_group_deltas(self, deltas):
        """deltas: iterable of (index, matched, status_scheduled, flags) — bs_groups_apply."""
        deltas = list(deltas)
        arr = (soa.GroupDelta * max(len(deltas), 1))(*[soa.GroupDelta(*map(int, d)) for d in deltas])
        self._chk(self._lib.bs_groups_apply(self._h, arr, len(deltas)), "bs_groups_apply")

    def filter_rows_count(self) -> int:
        n = C.c_uint32(0)
        self._chk(self._lib.bs_filter_rows_count(self._h, C.byref(n)), "bs_filter_rows_count")
        return int(n.value)

    def load_queue_order(self, order_rank):
        """per group: dense rank of (CreationTimestamp ascending, group name descending) — bs_queue_order_load"""
        r = np.ascontiguousarray(order_rank, dtype=np.uint32)
        self._chk(self._lib.bs_queue_order_load(self._h, len(r), _u32p(r if len(r) else np.zeros(1, np.uint32))), "bs_queue_order_load")

    def queue_sort(self, priority, group, queue_ts) -> np.ndarray:
        """the queue order ScheduleOperation.Compare (core.go:368-411) defines: perm[k] = pod at queue position k"""
        pr, gr, ts = (np.ascontiguousarray(priority, np.int32), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(queue_ts, np.int64))
        perm = np.zeros(max(len(pr), 1), np.uint32)
        self._chk(self._lib.bs_queue_sort(self._h, len(pr), pr.ctypes.data_as(C.POINTER(C.c_int32)), gr.ctypes.data_as(C.POINTER(C.c_int32)),
                                          _i64p(ts), _u32p(perm)), "bs_queue_sort")
        return perm[: len(pr)]

    def map_pods(self, p: int) -> soa.Pods:
        """Zero-copy hand-over (bs_pods_map): a Pods whose arrays ARE the library's pinned upload buffer.  Fill them in
        place and pass the object to load_pods — no packing copy.  Valid until the next map_pods / load_pods."""
        st = soa.PodsStruct()
        self._chk(self._lib.bs_pods_map(self._h, p, C.byref(st)), "bs_pods_map")

        def view(ptr, ctype, dtype, shape):
            n = int(np.prod(shape))
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype * n)).contents).view(dtype).reshape(shape)
        pods = soa.Pods.__new__(soa.Pods)
        pods.group = view(st.group, C.c_int32, np.int32, (p,))
        pods.req = view(st.req, C.c_int64, np.int64, (self.L, p))
        pods.req_present = view(st.req_present, C.c_uint32, np.uint32, (p,))
        pods.cls = view(st.cls, C.c_uint32, np.uint32, (p,))
        pods.owner = view(st.owner, C.c_uint64, np.uint64, (p,))
        pods.flags = view(st.flags, C.c_uint8, np.uint8, (p,))
        return pods

    def apply_group_deltas_raw(self, arr, n: int):
        """bs_groups_apply with a prebuilt (GroupDelta * n) array (no per-call marshalling)"""
        self._chk(self._lib.bs_groups_apply(self._h, arr, n), "bs_groups_apply")

    def load_pods(self, pods: soa.Pods):
        assert pods.req.shape[0] == self.L
        st = pods.as_struct()
        self._chk(self._lib.bs_pods_load(self._h, C.byref(st)), "bs_pods_load")
        self.p = pods.p

    def apply_pods(self, remove=(), flag_index=(), flag_value=(), insert: soa.Pods | None = None, insert_at=None):
        """bs_pods_apply: patch the resident queue on the device (stable removals, flag updates, insertions)."""
        rem = np.ascontiguousarray(remove, np.uint32)
        fi = np.ascontiguousarray(flag_index, np.uint32)
        fv = np.ascontiguousarray(flag_value, np.uint8)
        assert fi.shape == fv.shape
        d = soa.PodsDeltaStruct()
        d.n_remove, d.remove = len(rem), _u32p(rem if len(rem) else np.zeros(1, np.uint32))
        d.n_flags, d.flag_index = len(fi), _u32p(fi if len(fi) else np.zeros(1, np.uint32))
        d.flag_value = (fv if len(fv) else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8))
        keep = [rem, fi, fv]
        if insert is not None and insert.p:
            assert insert.req.shape[0] == self.L
            d.insert = insert.as_struct()
            if insert_at is not None:
                at = np.ascontiguousarray(insert_at, np.uint32)
                assert len(at) == insert.p
                keep.append(at)
                d.insert_at = _u32p(at)
        self._chk(self._lib.bs_pods_apply(self._h, C.byref(d)), "bs_pods_apply")
        self.p = self.pods_count()

    def apply_pods_raw(self, delta: "soa.PodsDeltaStruct"):
        """bs_pods_apply with a prebuilt struct (no per-call marshalling); the caller tracks p"""
        self._chk(self._lib.bs_pods_apply(self._h, C.byref(delta)), "bs_pods_apply")

    def apply_stats(self) -> tuple[int, int]:
        a, r = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._lib.bs_pods_apply_stats(self._h, C.byref(a), C.byref(r)), "bs_pods_apply_stats")
        return int(a.value), int(r.value)

    def speculation_stats(self) -> tuple[int, int]:
        """(batches launched on a guessed findMaxPG answer, wrong guesses that were re-run) — bs_speculation_stats"""
        a, m = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._lib.bs_speculation_stats(self._h, C.byref(a), C.byref(m)), "bs_speculation_stats")
        return int(a.value), int(m.value)

    def filter_deny_reruns(self) -> int:
        """BS_BATCH_FILTER_DENY batches that had to be run again so far (fixed-point iteration, bs_filter_deny_stats)"""
        r = C.c_uint64(0)
        self._chk(self._lib.bs_filter_deny_stats(self._h, C.byref(r)), "bs_filter_deny_stats")
        return int(r.value)

    def pods_count(self) -> int:
        n = C.c_uint32(0)
        self._chk(self._lib.bs_pods_count(self._h, C.byref(n)), "bs_pods_count")
        return int(n.value)

    def read_pods(self) -> soa.Pods:
        """the resident queue (bs_pods_read)"""
        p = self.pods_count()
        out = soa.Pods.empty(max(p, 1), self.L)
        st = soa.PodsOutStruct(p, *[getattr(out.as_struct(), k) for k in ("group", "req", "req_present", "cls", "owner", "flags")])
        if p:
            # the [L][p] lane stride must be p: read into exactly-sized arrays
            out = soa.Pods.empty(p, self.L)
            s2 = out.as_struct()
            st = soa.PodsOutStruct(p, s2.group, s2.req, s2.req_present, s2.cls, s2.owner, s2.flags)
        self._chk(self._lib.bs_pods_read(self._h, C.byref(st)), "bs_pods_read")
        return out if p else soa.Pods.empty(0, self.L)

    def apply_node_deltas(self, deltas: list):
        arr = (NodeDelta * len(deltas))(*deltas)
        self._chk(self._lib.bs_nodes_apply(self._h, arr, len(deltas)), "bs_nodes_apply")
        n = C.c_uint32(0)
        self._chk(self._lib.bs_nodes_count(self._h, C.byref(n)), "bs_nodes_count")
        self.n = int(n.value)

    def assume_nodes(self, reqs):
        """bs_nodes_assume: reqs = iterable of (node index, requested lanes, requested_present)"""
        reqs = list(reqs)
        arr = (NodeRequest * max(len(reqs), 1))()
        for k, (idx, lanes, pres) in enumerate(reqs):
            arr[k].index, arr[k].requested_present = int(idx), int(pres)
            for j, v in enumerate(lanes):
                arr[k].requested[j] = int(v)
        self._chk(self._lib.bs_nodes_assume(self._h, arr, len(reqs)), "bs_nodes_assume")

    # -- single queries
    def cluster_fits(self, cls: int, pct: float, req, present: int = 0):
        r = np.zeros(soa.MAX_LANES, np.int64)
        r[: len(req)] = req
        fits, fk = C.c_uint8(0), C.c_uint32(0)
        self._chk(self._lib.bs_cluster_fits(self._h, cls, float(np.float32(pct)), _i64p(r), present, C.byref(fits), C.byref(fk)),
                  "bs_cluster_fits")
        return bool(fits.value), int(fk.value)

    def node_left(self, cls: int, pct: float):
        left = np.zeros((self.L, self.n), np.int64)
        present = np.zeros(max(self.n, 1), np.uint32)
        self._chk(self._lib.bs_node_left(self._h, cls, float(np.float32(pct)), _i64p(left), _u32p(present)), "bs_node_left")
        return left, present[: self.n]

    def scan_prefix(self, cls: int, pct: float):
        n = max(self.n, 1)
        prefix = np.zeros((self.L, n), np.int64)
        present, idx = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        rows = C.c_uint32(0)
        self._chk(self._lib.bs_scan_prefix(self._h, cls, float(np.float32(pct)), _i64p(prefix), _u32p(present), _u32p(idx), C.byref(rows)),
                  "bs_scan_prefix")
        r = int(rows.value)
        return prefix[:, :r].copy(), present[:r].copy(), idx[:r].copy()

    def cluster_total(self, cls: int):
        tot = np.zeros(soa.MAX_LANES, np.int64)
        pr = C.c_uint32(0)
        self._chk(self._lib.bs_cluster_total(self._h, cls, _i64p(tot), C.byref(pr)), "bs_cluster_total")
        return tot[: self.L].tolist(), int(pr.value)

    def filter_one(self, pod_group: int, req, present: int, leader: int, node: int):
        r = np.zeros(soa.MAX_LANES, np.int64)
        r[: len(req)] = req
        fl, fn = C.c_uint8(0), C.c_uint8(0)
        self._chk(self._lib.bs_filter_one(self._h, pod_group, _i64p(r), present, leader, node, C.byref(fl), C.byref(fn)), "bs_filter_one")
        return int(fl.value), int(fn.value)

    def find_max_pg(self):
        leader, fin, pan = C.c_int32(0), C.c_uint32(0), C.c_uint8(0)
        self._chk(self._lib.bs_find_max_pg(self._h, C.byref(leader), C.byref(fin), C.byref(pan)), "bs_find_max_pg")
        return int(leader.value), bool(pan.value)

    # -- batch
    def run(self, stages: int = soa.STAGE_ALL):
        self._chk(self._lib.bs_batch_run(self._h, stages), "bs_batch_run")

    def sync(self):
        self._chk(self._lib.bs_batch_sync(self._h), "bs_batch_sync")

    def finish(self):
        self._chk(self._lib.bs_batch_finish(self._h), "bs_batch_finish")

    def read(self, bitmap: bool = True, out: soa.BatchOut | None = None, rows: bool | None = None) -> soa.BatchOut:
        """Copy the results of the last batch to the host (into `out` when given: no allocation).
        rows: also the Filter slot rows (fl_rows / fl_slot; default: whenever the bitmap is asked for);
        bitmap: the expanded pods x nodes bitmap (opt-in on the library side)."""
        if rows is None:
            rows = bitmap
        if out is None:
            out = soa.BatchOut.alloc(self.p, self.g, self.n, bitmap=bitmap, rows_cap=max(self.filter_rows_count(), 1) if rows else 0)
        st = out.as_struct()
        self._chk(self._lib.bs_batch_read(self._h, C.byref(st)), "bs_batch_read")
        return out

    def map_raw(self, view: soa.BatchViewStruct | None = None) -> soa.BatchViewStruct:
        """bs_batch_map: wait for the latency-mode batch and return the pointer view (no copy of any kind)."""
        if view is None:
            view = soa.BatchViewStruct()
        self._chk(self._lib.bs_batch_map(self._h, C.byref(view)), "bs_batch_map")
        return view

    def map_results(self) -> dict:
        """bs_batch_map as numpy views over the pinned result memory (valid until the next run)."""
        v = self.map_raw()
        arr = np.ctypeslib.as_array

        def a(ptr, n):
            return arr(ptr, shape=(n,)) if n and ptr else None
        out = {"p": v.p, "g": v.g, "pf_code": a(v.pf_code, v.p), "pf_first_k": a(v.pf_first_k, v.p), "pf_leader": a(v.pf_leader, v.p),
               "fl_code": a(v.fl_code, v.p), "fl_feasible": a(v.fl_feasible, v.p), "fl_slot": a(v.fl_slot, v.p),
               "group_admit": a(v.group_admit, v.g), "group_ready": a(v.group_ready, v.g), "fl_rows_n": v.fl_rows_n, "fl_rows": None, "fl_rows_feasible": None}
        if v.fl_rows and v.fl_rows_n:
            out["fl_rows"] = arr(v.fl_rows, shape=(v.words, v.fl_rows_stride))[:, : v.fl_rows_n]
            out["fl_rows_feasible"] = arr(v.fl_rows_feasible, shape=(v.fl_rows_n,))
        return out

    def batch(self, stages: int = soa.STAGE_ALL, bitmap: bool = True, rows: bool | None = None) -> soa.BatchOut:
        self.run(stages)
        return self.read(bitmap=bitmap, rows=rows)

    # -- the sequential pass
    def seq_run(self, stages: int = soa.STAGE_PREFILTER, cap: int | None = None) -> dict:
        """bs_seq_run: the reference's pod-by-pod cycle (PreFilter -> node choice -> assume -> Permit -> release) over the
        resident queue, on the device.  The context's node requests and group state are what the pass left."""
        return self._seq_pass(stages, cap, None, False)

    def _seq_pass(self, stages: int, cap, nominated, flat: bool, weights=None, sample=None) -> dict:
        """the result arrays of a sequential pass and the call: bs_seq_run (nominated None), else bs_seq_run_nominated with
        nominated = (p, priority, own_id), through its flat form when flat; weights = (w_least, w_most, w_balanced): bs_seq_run_scored; both:
        bs_seq_run_scored_nominated; sample = (num_to_find, start) on top of weights: the two sampled forms (rule F), "null": a NULL sample"""
        p, cap = self.pods_count(), max(self.g if cap is None else cap, 1)
        n = max(p, 1)
        pf, fk = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        ld, node = np.zeros(n, np.int32), np.full(n, -1, np.int32)
        rg, rp = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        t0, t1 = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        lp = np.zeros(n, np.uint8)
        o = SeqOut(pf.ctypes.data_as(C.POINTER(C.c_uint8)), _u32p(fk), ld.ctypes.data_as(C.POINTER(C.c_int32)), node.ctypes.data_as(C.POINTER(C.c_int32)),
                   cap, _u32p(rg), _u32p(rp), _i64p(t0), _i64p(t1), 0, 0, 0, 0, 0, 0, 0, 0, lp.ctypes.data_as(C.POINTER(C.c_uint8)))
        if sample is not None and flat:
            sc = np.zeros(8, np.int64)
            res = (o.pf_code, o.pf_first_k, o.pf_leader, o.pod_node, cap, o.released_group, o.released_pods, o.first_ns, o.ready_ns, _i64p(sc), o.last_permitted)
            if nominated is not None:
                self._chk(self._lib.bs_seq_run_scored_nominated_sampled_flat(self._h, stages, *nominated, *weights, *sample, *res), "bs_seq_run_scored_nominated_sampled_flat")
            else:
                self._chk(self._lib.bs_seq_run_scored_sampled_flat(self._h, stages, *weights, *sample, *res), "bs_seq_run_scored_sampled_flat")
            (o.n_released, o.total_ns, o.node_picks, o.node_scans, o.scan_rounds, o.pick_rounds, o.leader_folds, o.table_builds) = (int(v) for v in sc)
        elif sample is not None:
            w = None if weights == "null" else SeqScore(*weights)
            sm = None if sample == "null" else SeqSample(*sample)
            wp, sp = (None if w is None else C.byref(w)), (None if sm is None else C.byref(sm))
            if nominated is not None:
                self._chk(self._lib.bs_seq_run_scored_nominated_sampled(self._h, stages, *nominated, wp, sp, C.byref(o)), "bs_seq_run_scored_nominated_sampled")
            else:
                self._chk(self._lib.bs_seq_run_scored_sampled(self._h, stages, wp, sp, C.byref(o)), "bs_seq_run_scored_sampled")
        elif weights is not None and nominated is not None and flat:
            sc = np.zeros(8, np.int64)
            self._chk(self._lib.bs_seq_run_scored_nominated_flat(self._h, stages, *nominated, *weights, o.pf_code, o.pf_first_k, o.pf_leader, o.pod_node, cap,
                                                                 o.released_group, o.released_pods, o.first_ns, o.ready_ns, _i64p(sc), o.last_permitted),
                      "bs_seq_run_scored_nominated_flat")
            (o.n_released, o.total_ns, o.node_picks, o.node_scans, o.scan_rounds, o.pick_rounds, o.leader_folds, o.table_builds) = (int(v) for v in sc)
        elif weights is not None and nominated is not None:
            w = None if weights == "null" else SeqScore(*weights)
            self._chk(self._lib.bs_seq_run_scored_nominated(self._h, stages, *nominated, None if w is None else C.byref(w), C.byref(o)),
                      "bs_seq_run_scored_nominated")
        elif weights is not None and flat:
            sc = np.zeros(8, np.int64)
            self._chk(self._lib.bs_seq_run_scored_flat(self._h, stages, *weights, o.pf_code, o.pf_first_k, o.pf_leader, o.pod_node, cap, o.released_group,
                                                       o.released_pods, o.first_ns, o.ready_ns, _i64p(sc), o.last_permitted), "bs_seq_run_scored_flat")
            (o.n_released, o.total_ns, o.node_picks, o.node_scans, o.scan_rounds, o.pick_rounds, o.leader_folds, o.table_builds) = (int(v) for v in sc)
        elif weights is not None:
            w = SeqScore(*weights)
            self._chk(self._lib.bs_seq_run_scored(self._h, stages, C.byref(w), C.byref(o)), "bs_seq_run_scored")
        elif nominated is None:
            self._chk(self._lib.bs_seq_run(self._h, stages, C.byref(o)), "bs_seq_run")
        elif flat:
            sc = np.zeros(8, np.int64)
            self._chk(self._lib.bs_seq_run_nominated_flat(self._h, stages, *nominated, o.pf_code, o.pf_first_k, o.pf_leader, o.pod_node, cap, o.released_group,
                                                          o.released_pods, o.first_ns, o.ready_ns, _i64p(sc), o.last_permitted), "bs_seq_run_nominated_flat")
            (o.n_released, o.total_ns, o.node_picks, o.node_scans, o.scan_rounds, o.pick_rounds, o.leader_folds, o.table_builds) = (int(v) for v in sc)
        else:
            self._chk(self._lib.bs_seq_run_nominated(self._h, stages, *nominated, C.byref(o)), "bs_seq_run_nominated")
        k = min(int(o.n_released), cap)
        return dict(pf_code=pf[:p], pf_first_k=fk[:p], pf_leader=ld[:p], pod_node=node[:p], last_permitted=lp[:p], released_group=rg[:k], released_pods=rp[:k],
                    first_ns=t0[:k], ready_ns=t1[:k], n_released=int(o.n_released), total_ns=int(o.total_ns), node_picks=int(o.node_picks),
                    node_scans=int(o.node_scans), scan_rounds=int(o.scan_rounds), pick_rounds=int(o.pick_rounds), leader_folds=int(o.leader_folds), table_builds=int(o.table_builds))

    def seq_run_nominated(self, priority, own_id=None, stages: int = soa.STAGE_PREFILTER, cap: int | None = None, p: int | None = None,
                          flat: bool = False) -> dict:
        """bs_seq_run_nominated: seq_run with the resident nominated-pod table in the node choice (rule S).  priority[i]: the priority of
        queue pod i (None: a NULL array); own_id[i]: the id of the table row that IS pod i, NOM_NONE where it has none (None: a NULL
        array, nobody has one).  Rows whose pods were assumed leave the table (seq_nominated_read lists them).  p overrides the queue
        length handed to the library (tests of the refusals)."""
        pr = None if priority is None else np.ascontiguousarray(np.asarray(priority, np.int32).reshape(-1))
        ow = None if own_id is None else np.ascontiguousarray(np.asarray(own_id, np.uint32).reshape(-1))
        n = self.pods_count() if p is None else int(p)
        assert p is not None or ((pr is None or pr.size == n) and (ow is None or ow.size == n))
        pp = None if pr is None else (pr if pr.size else np.zeros(1, np.int32)).ctypes.data_as(C.POINTER(C.c_int32))
        op = None if ow is None else _u32p(ow if ow.size else np.zeros(1, np.uint32))
        return self._seq_pass(stages, cap, (n, pp, op), flat)

    def seq_run_scored_nominated(self, weights, priority, own_id=None, stages: int = soa.STAGE_PREFILTER, cap: int | None = None, p: int | None = None,
                                 flat: bool = False) -> dict:
        """bs_seq_run_scored_nominated: seq_run_scored with rule S in its candidate set and the consume behind its choice (rule SP).  The
        nominated-pod table narrows the candidates and never moves a score; weights as in seq_run_scored (None: a NULL score, tests of
        the refusals), priority / own_id / p as in seq_run_nominated.  seq_score_read and seq_nominated_read both answer for this pass."""
        pr = None if priority is None else np.ascontiguousarray(np.asarray(priority, np.int32).reshape(-1))
        ow = None if own_id is None else np.ascontiguousarray(np.asarray(own_id, np.uint32).reshape(-1))
        n = self.pods_count() if p is None else int(p)
        assert p is not None or ((pr is None or pr.size == n) and (ow is None or ow.size == n))
        pp = None if pr is None else (pr if pr.size else np.zeros(1, np.int32)).ctypes.data_as(C.POINTER(C.c_int32))
        op = None if ow is None else _u32p(ow if ow.size else np.zeros(1, np.uint32))
        assert not (weights is None and flat), "the flat form has no NULL score"
        w = "null" if weights is None else tuple(int(v) for v in weights)
        return self._seq_pass(stages, cap, (n, pp, op), flat, w)

    def seq_nominated_read(self, cap: int | None = None) -> dict:
        """bs_seq_nominated_read: the rows the last seq_run_nominated consumed, ascending id: n (the true count), id, pod (queue index), node
        (at most cap rows; the default holds every row the table had room for)."""
        cap = NOM_MAX if cap is None else int(cap)
        i_, pd, nd = (np.zeros(max(cap, 1), np.uint32) for _ in range(3))
        n = C.c_uint32(0)
        self._chk(self._lib.bs_seq_nominated_read(self._h, cap, _u32p(i_), _u32p(pd), _u32p(nd), C.byref(n)), "bs_seq_nominated_read")
        k = min(int(n.value), cap)
        return dict(n=int(n.value), id=i_[:k].copy(), pod=pd[:k].copy(), node=nd[:k].copy())

    def seq_run_scored(self, weights, stages: int = soa.STAGE_PREFILTER, cap: int | None = None, flat: bool = False) -> dict:
        """bs_seq_run_scored: seq_run with the node choice of rule P — among the nodes seq_run's rule accepts, the one with the largest
        w_least * least + w_most * most + w_balanced * balanced, ties to the lowest index.  weights = (w_least, w_most, w_balanced), each at
        most SCORE_WEIGHT_MAX; (0, 0, 0) is seq_run.  seq_score_read reports the chosen totals."""
        wl, wm, wb = (int(v) for v in weights)
        return self._seq_pass(stages, cap, None, flat, (wl, wm, wb))

    @staticmethod
    def _sample_arg(weights, sample, flat):
        assert not ((weights is None or sample is None) and flat), "the flat forms have no NULL score and no NULL sample"
        w = "null" if weights is None else tuple(int(v) for v in weights)
        s = "null" if sample is None else tuple(int(v) & 0xFFFFFFFF for v in sample)
        assert w == "null" or len(w) == 3
        assert s == "null" or len(s) == 2
        return w, s

    def seq_run_scored_sampled(self, weights, sample, stages: int = soa.STAGE_PREFILTER, cap: int | None = None, flat: bool = False) -> dict:
        """bs_seq_run_scored_sampled: seq_run_scored with upstream's node sampling (rule F).  sample = (num_to_find, start): the walk of
        every pod starts at a cursor that rotates from pod to pod (the first at start mod N), stops behind num_to_find candidates (0 or
        >= N: all) and scores those; ties go to the smallest visit position.  None for weights / sample: a NULL pointer (tests of the
        refusals).  seq_score_read (n_fit = the candidates kept) and seq_sample_read answer for this pass."""
        w, s = self._sample_arg(weights, sample, flat)
        return self._seq_pass(stages, cap, None, flat, w, s)

    def seq_run_scored_nominated_sampled(self, weights, sample, priority, own_id=None, stages: int = soa.STAGE_PREFILTER, cap: int | None = None,
                                         p: int | None = None, flat: bool = False) -> dict:
        """bs_seq_run_scored_nominated_sampled: seq_run_scored_nominated with rule F's walk over rule S's candidates.  sample as in
        seq_run_scored_sampled, the other arguments as in seq_run_scored_nominated.  seq_score_read, seq_sample_read and
        seq_nominated_read all answer for this pass."""
        pr = None if priority is None else np.ascontiguousarray(np.asarray(priority, np.int32).reshape(-1))
        ow = None if own_id is None else np.ascontiguousarray(np.asarray(own_id, np.uint32).reshape(-1))
        n = self.pods_count() if p is None else int(p)
        assert p is not None or ((pr is None or pr.size == n) and (ow is None or ow.size == n))
        pp = None if pr is None else (pr if pr.size else np.zeros(1, np.int32)).ctypes.data_as(C.POINTER(C.c_int32))
        op = None if ow is None else _u32p(ow if ow.size else np.zeros(1, np.uint32))
        w, s = self._sample_arg(weights, sample, flat)
        return self._seq_pass(stages, cap, (n, pp, op), flat, w, s)

    def seq_sample_read(self, p: int | None = None) -> dict:
        """bs_seq_sample_read: per queue pod of the last sampled pass the cursor its walk began at (0: the choice was not reached) and the
        nodes it visited, and next_start, the cursor behind the last pod — the next pass's sample start.  p overrides the queue length
        handed to the library (tests)."""
        n = self.pods_count() if p is None else int(p)
        start, visited = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        nxt = C.c_uint32(0)
        self._chk(self._lib.bs_seq_sample_read(self._h, n, _u32p(start), _u32p(visited), C.byref(nxt)), "bs_seq_sample_read")
        return dict(start=start[:n], visited=visited[:n], next_start=int(nxt.value))

    def seq_score_read(self, p: int | None = None) -> dict:
        """bs_seq_score_read: per queue pod of the last seq_run_scored the chosen node's total (0: no node) and n_fit, the number of nodes
        the node rule accepted (0: the choice was not reached).  p overrides the queue length handed to the library (tests)."""
        n = self.pods_count() if p is None else int(p)
        total, n_fit = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        self._chk(self._lib.bs_seq_score_read(self._h, n, _u32p(total), _u32p(n_fit)), "bs_seq_score_read")
        return dict(total=total[:n], n_fit=n_fit[:n])

    def seq_expire(self, groups=None, deny: bool = False, all: bool = False, group_cap: int | None = None, pod_cap: int | None = None,
                   flat: bool = False, flags: int | None = None) -> dict:
        """bs_seq_expire: the Permit timeout of the listed gangs (all=True: of every gang with waiting pods) — their waiting pods of the
        last seq_run leave their nodes, matched returns to 0, deny=True deny-lists the groups.  Returns n_groups, n_pods (true counts) and
        group, group_pods, group_earlier, pod, node (at most group_cap / pod_cap rows; the defaults hold everything).  flags overrides
        the flag word built from deny / all; flat=True goes through bs_seq_expire_flat."""
        gl = None if groups is None else np.ascontiguousarray(np.asarray(groups, np.uint32).reshape(-1))
        fl = ((SEQ_EXPIRE_DENY if deny else 0) | (SEQ_EXPIRE_ALL if all else 0)) if flags is None else int(flags)
        gcap = (self.g if gl is None else int(gl.size)) if group_cap is None else int(group_cap)
        pcap = self.pods_count() if pod_cap is None else int(pod_cap)
        g, gp, ge = (np.zeros(max(gcap, 1), np.uint32) for _ in range(3))
        pod, node = np.zeros(max(pcap, 1), np.uint32), np.zeros(max(pcap, 1), np.uint32)
        count = 0 if gl is None else int(gl.size)
        gptr = None if gl is None else _u32p(gl if gl.size else np.zeros(1, np.uint32))
        if flat:
            cnt = np.zeros(2, np.uint32)
            self._chk(self._lib.bs_seq_expire_flat(self._h, count, gptr, fl, gcap, _u32p(g), _u32p(gp), _u32p(ge), pcap, _u32p(pod), _u32p(node), _u32p(cnt)),
                      "bs_seq_expire_flat")
            ng, npods = int(cnt[0]), int(cnt[1])
        else:
            o = SeqExpireOut(0, 0, gcap, _u32p(g), _u32p(gp), _u32p(ge), pcap, _u32p(pod), _u32p(node))
            self._chk(self._lib.bs_seq_expire(self._h, count, gptr, fl, C.byref(o)), "bs_seq_expire")
            ng, npods = int(o.n_groups), int(o.n_pods)
        kg, kp = min(ng, gcap), min(npods, pcap)
        return dict(n_groups=ng, n_pods=npods, group=g[:kg], group_pods=gp[:kg], group_earlier=ge[:kg], pod=pod[:kp], node=node[:kp])

    def seq_waiting_read(self) -> np.ndarray:
        """bs_seq_waiting_read: per queue pod the node it still waits on after the last seq_run (and the expires since), else -1"""
        p = self.pods_count()
        wn = np.full(max(p, 1), -1, np.int32)
        self._chk(self._lib.bs_seq_waiting_read(self._h, p, wn.ctypes.data_as(C.POINTER(C.c_int32))), "bs_seq_waiting_read")
        return wn[:p]

    # -- the resident Permit-wait table
    def wait_load(self, node=(), group=(), req=None, req_present=None, w: int | None = None):
        """bs_wait_load: a fresh table of waiting pods (node [w], group [w], req [L][w], req_present [w]); no arguments: the empty table.
        w overrides the row count handed to the library (tests of the capacity check)."""
        nd = np.ascontiguousarray(np.asarray(node, np.uint32).reshape(-1))
        n = int(nd.size)
        gr = np.ascontiguousarray(np.asarray(group, np.int32).reshape(-1))
        rq = np.zeros((self.L, n), np.int64) if req is None else np.ascontiguousarray(np.asarray(req, np.int64).reshape(self.L, n))
        pr = np.zeros(n, np.uint32) if req_present is None else np.ascontiguousarray(np.asarray(req_present, np.uint32).reshape(-1))
        assert gr.size == n and pr.size == n
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)
        self._chk(self._lib.bs_wait_load(self._h, n if w is None else int(w), _u32p(pad(nd)), pad(gr).ctypes.data_as(C.POINTER(C.c_int32)), _i64p(pad(rq)),
                                         _u32p(pad(pr))), "bs_wait_load")

    def wait_count(self) -> int:
        w = C.c_uint32(0)
        self._chk(self._lib.bs_wait_count(self._h, C.byref(w)), "bs_wait_count")
        return int(w.value)

    def wait_ids(self) -> int:
        """bs_wait_ids: the id space — rows at the last wait_load plus what wait_park added since"""
        w = C.c_uint32(0)
        self._chk(self._lib.bs_wait_ids(self._h, C.byref(w)), "bs_wait_ids")
        return int(w.value)

    def wait_read(self) -> dict:
        """bs_wait_read: the table's columns in table order (ascending id): id, node, group, req [L][count], req_present"""
        w = self.wait_count()
        m = max(w, 1)
        i_, nd, gr, pr = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.int32), np.zeros(m, np.uint32)
        rq = np.zeros((self.L, m), np.int64) if w == 0 else np.zeros((self.L, w), np.int64)
        self._chk(self._lib.bs_wait_read(self._h, _u32p(i_), _u32p(nd), gr.ctypes.data_as(C.POINTER(C.c_int32)), _i64p(rq), _u32p(pr)), "bs_wait_read")
        return dict(id=i_[:w], node=nd[:w], group=gr[:w], req=rq[:, :w], req_present=pr[:w])

    def wait_park(self, cap: int | None = None) -> dict:
        """bs_wait_park: the last pass's waiting pods move into the table.  Returns first_id, n (the true count) and pod, node (at most cap
        rows; the default holds everything: the queue length)."""
        cap = self.pods_count() if cap is None else int(cap)
        pod, node = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        first, n = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._lib.bs_wait_park(self._h, cap, _u32p(pod), _u32p(node), C.byref(first), C.byref(n)), "bs_wait_park")
        k = min(int(n.value), cap)
        return dict(first_id=int(first.value), n=int(n.value), pod=pod[:k], node=node[:k])

    def _wait_by_group(self, groups, cap, expire, flags):
        gl = np.ascontiguousarray(np.asarray(groups, np.uint32).reshape(-1))
        cap = self.wait_count() if cap is None else int(cap)
        i_, nd = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        ge, gu = np.zeros(max(gl.size, 1), np.uint32), np.zeros(max(gl.size, 1), np.uint32)
        n = C.c_uint32(0)
        gp = _u32p(gl if gl.size else np.zeros(1, np.uint32))
        if expire:
            self._chk(self._lib.bs_wait_expire(self._h, int(gl.size), gp, int(flags), cap, _u32p(i_), _u32p(nd), _u32p(ge), _u32p(gu), C.byref(n)), "bs_wait_expire")
        else:
            self._chk(self._lib.bs_wait_release(self._h, int(gl.size), gp, cap, _u32p(i_), _u32p(nd), _u32p(ge), C.byref(n)), "bs_wait_release")
        k = min(int(n.value), cap)
        out = dict(n=int(n.value), id=i_[:k], node=nd[:k], group_entries=ge[: gl.size])
        if expire:
            out["group_unknown"] = gu[: gl.size]
        return out

    def wait_release(self, groups, cap: int | None = None) -> dict:
        """bs_wait_release: the rows of the gangs a later pass released leave the table.  Returns n (true count), id, node (ascending id, at
        most cap rows; the default holds the whole table) and group_entries in the caller's order."""
        return self._wait_by_group(groups, cap, False, 0)

    def wait_expire(self, groups, deny: bool = False, cap: int | None = None, flags: int | None = None) -> dict:
        """bs_wait_expire: the Permit timeout of the listed gangs for the table's rows — they leave the table and their nodes, matched returns
        to 0, deny=True deny-lists the groups.  As wait_release, plus group_unknown.  flags overrides the flag word built from deny."""
        return self._wait_by_group(groups, cap, True, (SEQ_EXPIRE_DENY if deny else 0) if flags is None else flags)

    def wait_forget(self, ids) -> np.ndarray:
        """bs_wait_forget: single rows leave the table and their nodes, matched of their groups falls by 1 each.  Returns the node of each id."""
        il = np.ascontiguousarray(np.asarray(ids, np.uint32).reshape(-1))
        out = np.zeros(max(il.size, 1), np.uint32)
        self._chk(self._lib.bs_wait_forget(self._h, int(il.size), _u32p(il if il.size else np.zeros(1, np.uint32)), _u32p(out)), "bs_wait_forget")
        return out[: il.size]

    def wait_nodes_apply(self, kind, index, cap: int | None = None):
        """bs_wait_nodes_apply: the wait table follows the node-list surgery of the apply_node_deltas call(s) before it — kind and index are
        those deltas' fields, in order.  Rows on removed nodes leave (matched of their groups falls by 1 each), the others keep their ids and
        get their nodes' new indices.  Returns (ids, old_nodes, groups, n): the dropped rows in ascending id (at most cap; the default holds
        the whole table) and their true number."""
        kv = np.ascontiguousarray(np.asarray(kind, np.uint32).reshape(-1))
        iv = np.ascontiguousarray(np.asarray(index, np.uint32).reshape(-1))
        assert kv.size == iv.size
        cap = self.wait_count() if cap is None else int(cap)
        i_, nd, gr = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.int32)
        n = C.c_uint32(0)
        self._chk(self._lib.bs_wait_nodes_apply(self._h, int(kv.size), _u32p(kv) if kv.size else None, _u32p(iv) if iv.size else None, cap,
                                                _u32p(i_) if cap else None, _u32p(nd) if cap else None,
                                                gr.ctypes.data_as(C.POINTER(C.c_int32)) if cap else None, C.byref(n)), "bs_wait_nodes_apply")
        k = min(int(n.value), cap)
        return i_[:k].copy(), nd[:k].copy(), gr[:k].copy(), int(n.value)

    # -- the resident nominated-pod table
    def nominated_load(self, node=(), priority=(), req=None, req_present=None, m: int | None = None):
        """bs_nominated_load: a fresh table of nominees (node [m], priority [m], req [L][m], req_present [m]); no arguments: the empty table.
        m overrides the row count handed to the library (tests of the capacity check)."""
        nd = np.ascontiguousarray(np.asarray(node, np.uint32).reshape(-1))
        n = int(nd.size)
        pr = np.ascontiguousarray(np.asarray(priority, np.int32).reshape(-1))
        rq = np.zeros((self.L, n), np.int64) if req is None else np.ascontiguousarray(np.asarray(req, np.int64).reshape(self.L, n))
        ps = np.zeros(n, np.uint32) if req_present is None else np.ascontiguousarray(np.asarray(req_present, np.uint32).reshape(-1))
        assert pr.size == n and ps.size == n
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)
        self._chk(self._lib.bs_nominated_load(self._h, n if m is None else int(m), _u32p(pad(nd)), pad(pr).ctypes.data_as(C.POINTER(C.c_int32)),
                                              _i64p(pad(rq)), _u32p(pad(ps))), "bs_nominated_load")

    def nominated_count(self) -> int:
        m = C.c_uint32(0)
        self._chk(self._lib.bs_nominated_count(self._h, C.byref(m)), "bs_nominated_count")
        return int(m.value)

    def nominated_ids(self) -> int:
        """bs_nominated_ids: the id space — rows at the last nominated_load plus what was inserted since"""
        m = C.c_uint32(0)
        self._chk(self._lib.bs_nominated_ids(self._h, C.byref(m)), "bs_nominated_ids")
        return int(m.value)

    def nominated_read(self) -> dict:
        """bs_nominated_read: the table's columns in table order (ascending id): id, node, priority, req [L][count], req_present"""
        w = self.nominated_count()
        m = max(w, 1)
        i_, nd, pr, ps = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.int32), np.zeros(m, np.uint32)
        rq = np.zeros((self.L, m), np.int64)
        self._chk(self._lib.bs_nominated_read(self._h, _u32p(i_), _u32p(nd), pr.ctypes.data_as(C.POINTER(C.c_int32)), _i64p(rq), _u32p(ps)), "bs_nominated_read")
        return dict(id=i_[:w], node=nd[:w], priority=pr[:w], req=rq[:, :w], req_present=ps[:w])

    def nominated_apply(self, remove=(), pod_index=(), node=(), priority=(), n_remove: int | None = None, n_insert: int | None = None) -> int:
        """bs_nominated_apply: the listed ids leave the table; then one row per (pod_index[k], node[k], priority[k]) is appended, its request
        gathered on the device from the resident queue.  Returns the first new id.  n_remove / n_insert override the counts handed to the
        library (tests of the refusals); an empty list is passed as NULL."""
        rm = np.ascontiguousarray(np.asarray(remove, np.uint32).reshape(-1))
        pi = np.ascontiguousarray(np.asarray(pod_index, np.uint32).reshape(-1))
        nd = np.ascontiguousarray(np.asarray(node, np.uint32).reshape(-1))
        pr = np.ascontiguousarray(np.asarray(priority, np.int32).reshape(-1))
        assert pi.size == nd.size == pr.size
        first = C.c_uint32(0)
        self._chk(self._lib.bs_nominated_apply(self._h, int(rm.size) if n_remove is None else int(n_remove), _u32p(rm) if rm.size else None,
                                               int(pi.size) if n_insert is None else int(n_insert), _u32p(pi) if pi.size else None,
                                               _u32p(nd) if nd.size else None, pr.ctypes.data_as(C.POINTER(C.c_int32)) if pr.size else None,
                                               C.byref(first)), "bs_nominated_apply")
        return int(first.value)

    def nominated_nodes_apply(self, kind, index, cap: int | None = None):
        """bs_nominated_nodes_apply: the nominated-pod table follows the node-list surgery of the apply_node_deltas call(s) before it — kind
        and index are those deltas' fields, in order.  Rows on removed nodes leave (their ids are dead), the others keep their ids and get
        their nodes' new indices.  Returns (ids, old_nodes, priorities, n): the dropped rows in ascending id (at most cap; the default
        holds the whole table) and their true number."""
        kv = np.ascontiguousarray(np.asarray(kind, np.uint32).reshape(-1))
        iv = np.ascontiguousarray(np.asarray(index, np.uint32).reshape(-1))
        assert kv.size == iv.size
        cap = self.nominated_count() if cap is None else int(cap)
        i_, nd, pr = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.int32)
        n = C.c_uint32(0)
        self._chk(self._lib.bs_nominated_nodes_apply(self._h, int(kv.size), _u32p(kv) if kv.size else None, _u32p(iv) if iv.size else None, cap,
                                                     _u32p(i_) if cap else None, _u32p(nd) if cap else None,
                                                     pr.ctypes.data_as(C.POINTER(C.c_int32)) if cap else None, C.byref(n)), "bs_nominated_nodes_apply")
        k = min(int(n.value), cap)
        return i_[:k].copy(), nd[:k].copy(), pr[:k].copy(), int(n.value)

    def preempt_nominated_read(self, count: int) -> np.ndarray:
        """bs_preempt_nominated_read: the row id per preemptor of the last preemption call with nominate=True, NOM_NONE where none"""
        out = np.zeros(max(int(count), 1), np.uint32)
        self._chk(self._lib.bs_preempt_nominated_read(self._h, int(count), _u32p(out)), "bs_preempt_nominated_read")
        return out[: int(count)]

    def preempt_cleared_read(self, cap: int | None = None) -> dict:
        """bs_preempt_cleared_read: the rows of the nominated-pod table the last preemption call with clear_lower=True cleared, in ascending
        id: id, node, priority, by (the caller-order index of the preemptor that stands first on the row's node), and n, the true count
        (the columns hold min(n, cap) rows; cap None reads them all; cap 0 passes NULL columns)."""
        n = C.c_uint32(0)
        if cap is None:
            self._chk(self._lib.bs_preempt_cleared_read(self._h, 0, None, None, None, None, C.byref(n)), "bs_preempt_cleared_read")
            cap = int(n.value)
        cap = int(cap)
        m = max(cap, 1)
        i_, nd, pr, by = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.int32), np.zeros(m, np.uint32)
        self._chk(self._lib.bs_preempt_cleared_read(self._h, cap, _u32p(i_) if cap else None, _u32p(nd) if cap else None,
                                                    pr.ctypes.data_as(C.POINTER(C.c_int32)) if cap else None, _u32p(by) if cap else None,
                                                    C.byref(n)), "bs_preempt_cleared_read")
        k = min(int(n.value), cap)
        return dict(id=i_[:k].copy(), node=nd[:k].copy(), priority=pr[:k].copy(), by=by[:k].copy(), n=int(n.value))

    def read_node_requests(self):
        """bs_nodes_read: (requested [L][n], requested_present [n]) as the context holds them"""
        req = np.zeros((self.L, max(self.n, 1)), np.int64) if self.n == 0 else np.zeros((self.L, self.n), np.int64)
        pres = np.zeros(max(self.n, 1), np.uint32)
        self._chk(self._lib.bs_nodes_read(self._h, _i64p(req), _u32p(pres)), "bs_nodes_read")
        return req[:, : self.n], pres[: self.n]

    # -- preemption
    def load_bound(self, bound: soa.Bound):
        """bs_bound_load: the pods bound to or assumed on the loaded nodes (resident until the next load)."""
        assert bound.req.shape[0] == self.L, f"context has {self.L} lanes, bound pods have {bound.req.shape[0]}"
        st = bound.as_struct()
        self._chk(self._lib.bs_bound_load(self._h, C.byref(st)), "bs_bound_load")
        self._bound_ids = int(bound.b)

    def bound_count(self) -> int:
        b = C.c_uint32()
        self._chk(self._lib.bs_bound_count(self._h, C.byref(b)), "bs_bound_count")
        return int(b.value)

    def bound_pdb_set(self, violating, b: int | None = None):
        """bs_bound_pdb_set: violating[id] != 0 = evicting bound pod `id` (the numbering of the last load_bound) would violate a
        PodDisruptionBudget (pdb.violating_bits builds the array); None clears every bit.  b defaults to the array's length (to the
        last load's entry count for None)."""
        if violating is None:
            v, ptr = None, None
        else:
            v = np.ascontiguousarray(np.asarray(violating).reshape(-1) != 0, np.uint8)
            ptr = v.ctypes.data_as(C.POINTER(C.c_uint8)) if v.size else None
        if b is None:
            b = getattr(self, "_bound_ids", 0) if v is None else int(v.size)
        self._chk(self._lib.bs_bound_pdb_set(self._h, int(b), ptr), "bs_bound_pdb_set")

    def preempt(self, pod_index, priority, group_protected=None, victim_cap: int = 16, stages: int = soa.STAGE_PREFILTER) -> dict:
        """bs_preempt_run: the victim search for every preemptor (resident-queue pod pod_index[q] at priority[q]); group_protected[g]
        from `group_protected(phases)`.  Returns node, n_candidates, n_victims, victims [count, victim_cap] (zero beyond
        min(n_victims, cap)), top_priority, priority_sum, earliest_start, n_pdb_violations (bs_preempt_pdb_read)."""
        return self._preempt_call(None, pod_index, priority, group_protected, victim_cap, stages)

    def preempt_commit(self, pod_index, priority, group_protected=None, victim_cap: int = 16, apply: bool = False, assume: bool = False,
                       stages: int = soa.STAGE_PREFILTER, nominate: bool = False, clear_lower: bool = False) -> dict:
        """bs_preempt_commit: the preemptors answered in sequence (priority descending, stable), each seeing the earlier slots' victims
        gone and their preemptors nominated; apply=True writes the evictions into the bound table and the node requests, assume=True
        (with apply) also adds each nominee's request to its node; nominate=True (with apply, without assume) appends each nominee to the
        nominated-pod table instead, and the dict gains nominated_id [count] (NOM_NONE where none).  clear_lower=True (rule C): a slot
        that stands on a node clears the lower-priority rows of the nominated-pod table on it for the later slots (and, with apply, out
        of the table); the dict gains cleared = {id, node, priority, by}.  Returns the dict `preempt` returns."""
        flags = (soa.PREEMPT_APPLY if apply else 0) | (soa.PREEMPT_ASSUME if assume else 0) | (soa.PREEMPT_NOMINATE if nominate else 0)
        flags |= soa.PREEMPT_CLEAR_LOWER if clear_lower else 0
        res = self._preempt_call(flags, pod_index, priority, group_protected, victim_cap, stages)
        if nominate:
            res["nominated_id"] = self.preempt_nominated_read(len(res["node"]))
        if clear_lower:
            res["cleared"] = self._cleared()
        return res

    def _cleared(self) -> dict:
        c = self.preempt_cleared_read()
        return {f: c[f] for f in ("id", "node", "priority", "by")}

    def preempt_commit_gang(self, pod_index, priority, group_protected=None, gang_need=None, victim_cap: int = 16, apply: bool = False,
                            assume: bool = False, stages: int = soa.STAGE_PREFILTER, flat: bool = False, nominate: bool = False,
                            clear_lower: bool = False) -> dict:
        """bs_preempt_commit_gang: preempt_commit, with each gang's quorum decided inside the pass: gang_need[g] members of group g must
        get a node in this call (the module's gang_need builds it; gang_order makes each gang one run), or the gang's slots are voided
        and their evictions taken back before the later slots are answered.  Returns preempt_commit's dict plus slot_voided [count]
        and group_placed [g] (bs_preempt_gang_read).  flat=True goes through bs_preempt_commit_gang_flat.  clear_lower: as preempt_commit's
        (a voided run's clearings are taken back)."""
        flags = (soa.PREEMPT_APPLY if apply else 0) | (soa.PREEMPT_ASSUME if assume else 0) | (soa.PREEMPT_NOMINATE if nominate else 0)
        flags |= soa.PREEMPT_CLEAR_LOWER if clear_lower else 0
        need = None if gang_need is None else np.ascontiguousarray(np.asarray(gang_need, np.uint32).reshape(-1))
        res = self._preempt_call(flags, pod_index, priority, group_protected, victim_cap, stages, gang=(need, flat))
        q, g = len(res["node"]), 0 if need is None else int(need.size)
        voided, placed = np.zeros(max(q, 1), np.uint8), np.zeros(max(g, 1), np.uint32)
        self._chk(self._lib.bs_preempt_gang_read(self._h, q, voided.ctypes.data_as(C.POINTER(C.c_uint8)), g, _u32p(placed)), "bs_preempt_gang_read")
        res["slot_voided"], res["group_placed"] = voided[:q], placed[:g]
        if nominate:
            res["nominated_id"] = self.preempt_nominated_read(q)
        if clear_lower:
            res["cleared"] = self._cleared()
        return res

    def _preempt_call(self, flags, pod_index, priority, group_protected, victim_cap, stages, gang=None) -> dict:
        pi = np.ascontiguousarray(np.asarray(pod_index, np.uint32).reshape(-1))
        pr = np.ascontiguousarray(np.asarray(priority, np.int32).reshape(-1))
        assert pi.shape == pr.shape
        q = pi.shape[0]
        n = max(q, 1)
        gp = None if group_protected is None else np.ascontiguousarray(np.asarray(group_protected, np.uint8).reshape(-1))
        node, ncand, nv = np.full(n, -1, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        vic = np.zeros((n, max(victim_cap, 1)), np.uint32)
        top, ssum, est = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64)
        o = soa.PreemptOutStruct(node.ctypes.data_as(C.POINTER(C.c_int32)), _u32p(ncand), _u32p(nv), _u32p(vic),
                                 top.ctypes.data_as(C.POINTER(C.c_int32)), _i64p(ssum), _i64p(est))
        gptr = gp.ctypes.data_as(C.POINTER(C.c_uint8)) if gp is not None and gp.size else None
        if flags is None:
            self._chk(self._lib.bs_preempt_run(self._h, stages, q, _u32p(pi), pr.ctypes.data_as(C.POINTER(C.c_int32)), gptr, victim_cap, C.byref(o)),
                      "bs_preempt_run")
        elif gang is not None:
            need, flat = gang
            nptr = _u32p(need) if need is not None and need.size else None
            i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
            if flat:
                self._chk(self._lib.bs_preempt_commit_gang_flat(self._h, stages, q, _u32p(pi), i32p(pr), gptr, nptr, flags, victim_cap, i32p(node),
                                                                _u32p(ncand), _u32p(nv), _u32p(vic), i32p(top), _i64p(ssum), _i64p(est)),
                          "bs_preempt_commit_gang_flat")
            else:
                self._chk(self._lib.bs_preempt_commit_gang(self._h, stages, q, _u32p(pi), i32p(pr), gptr, nptr, flags, victim_cap, C.byref(o)),
                          "bs_preempt_commit_gang")
        else:
            self._chk(self._lib.bs_preempt_commit(self._h, stages, q, _u32p(pi), pr.ctypes.data_as(C.POINTER(C.c_int32)), gptr, flags, victim_cap,
                                                  C.byref(o)), "bs_preempt_commit")
        npv = np.zeros(n, np.uint32)
        self._chk(self._lib.bs_preempt_pdb_read(self._h, q, _u32p(npv)), "bs_preempt_pdb_read")
        return dict(node=node[:q], n_candidates=ncand[:q], n_victims=nv[:q], victims=vic[:q, :victim_cap], top_priority=top[:q],
                    priority_sum=ssum[:q], earliest_start=est[:q], n_pdb_violations=npv[:q])

    def read_bound(self):
        """bs_bound_read: the live bound table in table order (node ascending, importance order within a node) as (id, node)"""
        b = self.bound_count()
        ids, node = np.zeros(max(b, 1), np.uint32), np.zeros(max(b, 1), np.uint32)
        self._chk(self._lib.bs_bound_read(self._h, _u32p(ids), _u32p(node)), "bs_bound_read")
        return ids[:b], node[:b]

    def bound_ids(self) -> int:
        """bs_bound_ids: the size of the bound table's id space (the last load's entry count plus what bound_apply inserted since)"""
        v = C.c_uint32()
        self._chk(self._lib.bs_bound_ids(self._h, C.byref(v)), "bs_bound_ids")
        return int(v.value)

    def bound_apply_ex(self, remove=None, insert: "soa.Bound | None" = None, pdb=None, flags: int = BS_BOUND_NODES, flat: bool = False) -> int:
        """bs_bound_apply_ex: bound_apply with flags.  BS_BOUND_NODES (the default here): the node requests follow the delta on the
        device, RemovePod per removed entry and AddPod per inserted one; 0: exactly bound_apply.  flat=True goes through
        bs_bound_apply_ex_flat."""
        return self.bound_apply(remove, insert, pdb, flat=flat, flags=int(flags))

    def bound_apply(self, remove=None, insert: "soa.Bound | None" = None, pdb=None, flat: bool = False, flags: int | None = None) -> int:
        """bs_bound_apply: entries `remove` (ids) leave the resident bound table, the entries of `insert` arrive with ids
        first_id, first_id + 1, ... (pdb[i] != 0: inserted entry i is PDB-violating; None = clear).  Returns first_id.  flat=True goes
        through bs_bound_apply_flat (the cgo form).  flags not None: through bs_bound_apply_ex / _ex_flat with these flags."""
        rem = np.ascontiguousarray(np.asarray([] if remove is None else remove, np.uint32).reshape(-1))
        ni = 0 if insert is None else int(insert.b)
        if ni:
            assert insert.req.shape[0] == self.L, f"context has {self.L} lanes, inserted pods have {insert.req.shape[0]}"
        pv = None if pdb is None or ni == 0 else np.ascontiguousarray(np.asarray(pdb).reshape(-1) != 0, np.uint8)
        assert pv is None or pv.size == ni
        u8p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
        i32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        cols = (None,) * 6 if ni == 0 else (_u32p(insert.node), i32p(insert.priority), _i64p(insert.start_ns), i32p(insert.group),
                                            _i64p(np.ascontiguousarray(insert.req)), _u32p(insert.req_present))
        first = C.c_uint32()
        rp = _u32p(rem) if rem.size else None
        pp = u8p(pv) if pv is not None else None
        if flags is not None and flat:
            self._chk(self._lib.bs_bound_apply_ex_flat(self._h, flags, int(rem.size), rp, ni, *cols, pp, C.byref(first)), "bs_bound_apply_ex_flat")
        elif flags is not None:
            d = soa.BoundDeltaStruct(int(rem.size), rp, ni, *cols, pp)
            self._chk(self._lib.bs_bound_apply_ex(self._h, C.byref(d), flags, C.byref(first)), "bs_bound_apply_ex")
        elif flat:
            self._chk(self._lib.bs_bound_apply_flat(self._h, int(rem.size), rp, ni, *cols, pp, C.byref(first)), "bs_bound_apply_flat")
        else:
            d = soa.BoundDeltaStruct(int(rem.size), rp, ni, *cols, pp)
            self._chk(self._lib.bs_bound_apply(self._h, C.byref(d), C.byref(first)), "bs_bound_apply")
        self._bound_ids = int(first.value) + ni
        return int(first.value)

    def bound_bind(self, wait_ids, pod_index, priority, start_ns, pdb=None) -> dict:
        """bs_bound_bind: the listed rows of the wait table and the listed pods the last pass placed enter the resident bound table on the
        device (row i: the wait ids first, then the pods; priority[i], start_ns[i], pdb[i] != 0: PDB-violating, None = clear) and the wait
        rows leave their table.  Returns dict(first_id=the id of row 0, node=the node each row bound on)."""
        wl = np.ascontiguousarray(np.asarray([] if wait_ids is None else wait_ids, np.uint32).reshape(-1))
        pl = np.ascontiguousarray(np.asarray([] if pod_index is None else pod_index, np.uint32).reshape(-1))
        n = int(wl.size + pl.size)
        pr = np.ascontiguousarray(np.asarray(priority, np.int32).reshape(-1))
        st = np.ascontiguousarray(np.asarray(start_ns, np.int64).reshape(-1))
        assert pr.size == n and st.size == n, "priority and start_ns are per row: the wait rows first, then the pods"
        pv = None if pdb is None or n == 0 else np.ascontiguousarray(np.asarray(pdb).reshape(-1) != 0, np.uint8)
        assert pv is None or pv.size == n
        node = np.zeros(max(n, 1), np.uint32)
        first = C.c_uint32()
        self._chk(self._lib.bs_bound_bind(self._h, int(wl.size), _u32p(wl) if wl.size else None, int(pl.size), _u32p(pl) if pl.size else None,
                                          pr.ctypes.data_as(C.POINTER(C.c_int32)) if n else None, _i64p(st) if n else None,
                                          pv.ctypes.data_as(C.POINTER(C.c_uint8)) if pv is not None else None, _u32p(node), C.byref(first)),
                  "bs_bound_bind")
        return dict(first_id=int(first.value), node=node[:n].copy())

    def bound_nodes_apply(self, kind, index, dropped_cap: int = 0):
        """bs_bound_nodes_apply: the resident bound table follows the node-list surgery of the apply_node_deltas call(s) before it — kind
        and index are those deltas' fields, in order.  Returns (n_dropped, ids): the true number of entries that left with their nodes and
        the first min(n_dropped, dropped_cap) of their ids in the old table's order."""
        kv = np.ascontiguousarray(np.asarray(kind, np.uint32).reshape(-1))
        iv = np.ascontiguousarray(np.asarray(index, np.uint32).reshape(-1))
        assert kv.size == iv.size
        ids = np.zeros(max(int(dropped_cap), 1), np.uint32)
        nd = C.c_uint32()
        self._chk(self._lib.bs_bound_nodes_apply(self._h, int(kv.size), _u32p(kv) if kv.size else None, _u32p(iv) if iv.size else None,
                                                 int(dropped_cap), _u32p(ids) if dropped_cap else None, C.byref(nd)), "bs_bound_nodes_apply")
        return int(nd.value), ids[: min(int(nd.value), int(dropped_cap))].copy()

    # -- resident PodDisruptionBudgets: the PDB bits follow the budgets' status on the device
    def pdb_load(self, allowed, member_off, member, b: int | None = None):
        """bs_pdb_load: allowed[n_pdb] (Status.PodDisruptionsAllowed) and, per bound-pod id, the PDBs that select it as a CSR
        (pdb.matching_members / pdb.allowed_vector build the arrays).  b defaults to len(member_off) - 1 and must equal bound_ids()."""
        al = np.ascontiguousarray(allowed, np.int32).reshape(-1)
        off = np.ascontiguousarray(member_off, np.uint32).reshape(-1)
        mem = np.ascontiguousarray(member, np.uint32).reshape(-1)
        b = max(off.size - 1, 0) if b is None else int(b)
        self._chk(self._lib.bs_pdb_load(self._h, int(al.size), al.ctypes.data_as(C.POINTER(C.c_int32)) if al.size else None, b,
                                        _u32p(off) if off.size else None, _u32p(mem) if mem.size else None), "bs_pdb_load")

    def pdb_members_append(self, first_id: int, member_off, member):
        """bs_pdb_members_append: the memberships of ids first_id .. first_id + len(member_off) - 2, the ids bound_apply created since
        the CSR last covered the id space (member_off is the run's own, from 0)"""
        off = np.ascontiguousarray(member_off, np.uint32).reshape(-1)
        mem = np.ascontiguousarray(member, np.uint32).reshape(-1)
        self._chk(self._lib.bs_pdb_members_append(self._h, int(first_id), max(off.size - 1, 0), _u32p(off) if off.size else None,
                                                  _u32p(mem) if mem.size else None), "bs_pdb_members_append")

    def pdb_allowed_apply(self, index, value):
        """bs_pdb_allowed_apply: allowed[index[i]] = value[i], then the bits and per-node counts are recomputed on the device"""
        ix = np.ascontiguousarray(index, np.uint32).reshape(-1)
        va = np.ascontiguousarray(value, np.int32).reshape(-1)
        assert ix.size == va.size
        self._chk(self._lib.bs_pdb_allowed_apply(self._h, int(ix.size), _u32p(ix) if ix.size else None,
                                                 va.ctypes.data_as(C.POINTER(C.c_int32)) if va.size else None), "bs_pdb_allowed_apply")

    def pdb_read(self) -> dict:
        """bs_pdb_read: n_pdb, covered, allowed[n_pdb] and the live table's per-node violating counts"""
        n, cov = C.c_uint32(0), C.c_uint32(0)
        self._chk(self._lib.bs_pdb_read(self._h, C.byref(n), C.byref(cov), None, None), "bs_pdb_read")
        nodes = C.c_uint32(0)
        self._chk(self._lib.bs_nodes_count(self._h, C.byref(nodes)), "bs_nodes_count")
        al, nv = np.zeros(max(n.value, 1), np.int32), np.zeros(max(nodes.value, 1), np.uint32)
        self._chk(self._lib.bs_pdb_read(self._h, None, None, al.ctypes.data_as(C.POINTER(C.c_int32)), _u32p(nv)), "bs_pdb_read")
        return dict(n_pdb=int(n.value), covered=int(cov.value), allowed=al[: n.value], node_violating=nv[: nodes.value])

    def bound_dump(self) -> dict:
        """bs_bound_dump: the live table's columns as stored, in read_bound's order: priority, start_ns, group, req [L, count],
        req_present, pdb"""
        b = self.bound_count()
        n = max(b, 1)
        prio, start, grp = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32)
        req, pres, pdb = np.zeros((self.L, n), np.int64), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._chk(self._lib.bs_bound_dump(self._h, prio.ctypes.data_as(C.POINTER(C.c_int32)), _i64p(start), grp.ctypes.data_as(C.POINTER(C.c_int32)),
                                          _i64p(req), _u32p(pres), pdb.ctypes.data_as(C.POINTER(C.c_uint8))), "bs_bound_dump")
        return dict(priority=prio[:b], start_ns=start[:b], group=grp[:b], req=req[:, :b], req_present=pres[:b], pdb=pdb[:b])

    # -- sharding / measurement
    def set_shard(self, rank: int, nranks: int):
        self._chk(self._lib.bs_shard_set(self._h, rank, nranks), "bs_shard_set")

    def reduce_external(self, on: bool = True):
        self._chk(self._lib.bs_reduce_external(self._h, 1 if on else 0), "bs_reduce_external")

    def first_reach_hint(self, local_index: int):
        """bs_first_reach_hint: partitioned mode, this rank's pods in front of the job's first pod that reaches findMaxPG"""
        self._chk(self._lib.bs_first_reach_hint(self._h, int(local_index) & 0xFFFFFFFF), "bs_first_reach_hint")

    def admit_devptr(self):
        p, n = C.c_void_p(), C.c_uint32(0)
        self._chk(self._lib.bs_group_admit_devptr(self._h, C.byref(p), C.byref(n)), "bs_group_admit_devptr")
        return int(p.value or 0), int(n.value)

    def bind_admit(self, dptr: int | None):
        self._chk(self._lib.bs_group_admit_bind(self._h, C.c_void_p(dptr or 0)), "bs_group_admit_bind")

    def stream(self) -> int:
        p = C.c_void_p()
        self._chk(self._lib.bs_stream(self._h, C.byref(p)), "bs_stream")
        return int(p.value or 0)

    def comm_init(self, uid: bytes, rank: int, nranks: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._chk(self._lib.bs_comm_init(self._h, buf, rank, nranks), "bs_comm_init")

    def timing_reset(self):
        self._chk(self._lib.bs_timing_reset(self._h), "bs_timing_reset")

    def timing(self) -> dict:
        t = Timing()
        self._chk(self._lib.bs_timing_get(self._h, C.byref(t)), "bs_timing_get")
        return {self._lib.bs_kernel_name(i).decode(): (float(t.total_ms[i]), int(t.launches[i])) for i in range(KERNEL_COUNT)}

    def stats_arm(self):
        s = BatchStats()
        self._chk(self._lib.bs_batch_stats_get(self._h, C.byref(s)), "bs_batch_stats_get")

    def stats(self, stages: int = soa.STAGE_ALL) -> dict:
        """Work counters of one instrumented batch (arm, run, read)."""
        self.stats_arm()
        self.run(stages)
        self.sync()
        return self.stats_read()

    def stats_read(self) -> dict:
        s = BatchStats()
        self._chk(self._lib.bs_batch_stats_get(self._h, C.byref(s)), "bs_batch_stats_get")
        return {k: int(getattr(s, k)) for k, _ in BatchStats._fields_}


def comm_unique_id() -> bytes:
    lib = load_library()
    buf = (C.c_uint8 * 128)()
    rc = lib.bs_comm_unique_id(buf)
    if rc != 0:
        raise BsError(rc, "bs_comm_unique_id")
    return bytes(buf)


def seq_sample_size(n: int, percentage: int = 0) -> int:
    """bs_seq_sample_size: upstream's numFeasibleNodesToFind (D9 of include/bsched.h) for n nodes under percentageOfNodesToScore = percentage
    (0 or less: the adaptive default)."""
    return int(load_library().bs_seq_sample_size(int(n), int(percentage)))
