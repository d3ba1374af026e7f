"""Submit-limit inputs (include/crane_gpu_submit/submit_limits.h) as numpy tables + ctypes views.

Mirror of what `AccountMetaContainer::TryMallocMetaSubmitResource` / `MallocMetaSubmitResource` read and write
(src/CraneCtld/Accounting/AccountMetaContainer.cpp:75-153, :374-506, :694-889, :1067-1124): `SubmitTables` = the submit-side limits
of Qos and PartitionResourceLimit, the usage the DenyOnLimit checks read, the five submit_jobs_count tables and one exists byte per
user / account / QoS; `SubmitKeys` = what the job table of validity does not carry.  Pure plumbing: no admission logic here.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import abi
from .limits import LIM_NONE, TRES_DT, UNLIMITED_CPU_RAW, UNLIMITED_JOBS, coerce_tables, table_shapes, unlimited_tres

SUBMIT_QOS_DT = np.dtype([("max_submit_jobs_per_user", "<u4"), ("max_submit_jobs_per_account", "<u4"), ("max_submit_jobs", "<u4"),
                          ("max_jobs_per_user", "<u4"), ("max_jobs_per_account", "<u4"), ("max_jobs", "<u4"), ("deny_on_limit", "<u4"),
                          ("reserved0", "<u4"), ("max_cpus_per_user_raw", "<i8"), ("max_wall_sec", "<i8"), ("max_time_limit_per_job_sec", "<i8"),
                          ("max_tres", TRES_DT), ("max_tres_per_user", TRES_DT), ("max_tres_per_account", TRES_DT)])
SUBMIT_PART_LIMIT_DT = np.dtype([("max_submit_jobs", "<u4"), ("reserved0", "<u4"), ("max_wall_duration_per_job_sec", "<i8"),
                                 ("max_tres_per_job", TRES_DT)])
assert SUBMIT_QOS_DT.itemsize == 416 and SUBMIT_PART_LIMIT_DT.itemsize == 136


def submit_qos(max_submit_jobs_per_user=UNLIMITED_JOBS, max_submit_jobs_per_account=UNLIMITED_JOBS, max_submit_jobs=UNLIMITED_JOBS,
               max_jobs_per_user=UNLIMITED_JOBS, max_jobs_per_account=UNLIMITED_JOBS, max_jobs=UNLIMITED_JOBS, deny_on_limit=False,
               max_cpus_per_user=None, max_wall_sec=0, max_time_limit_per_job_sec=abi.SUBMIT_JOB_MAX_TIME_LIMIT_SEC, max_tres=None,
               max_tres_per_user=None, max_tres_per_account=None) -> np.ndarray:
    """A Qos with the reference's defaults: everything unlimited, DenyOnLimit off."""
    q = np.zeros((), SUBMIT_QOS_DT)
    q["max_submit_jobs_per_user"], q["max_submit_jobs_per_account"], q["max_submit_jobs"] = max_submit_jobs_per_user, max_submit_jobs_per_account, max_submit_jobs
    q["max_jobs_per_user"], q["max_jobs_per_account"], q["max_jobs"] = max_jobs_per_user, max_jobs_per_account, max_jobs
    q["deny_on_limit"] = 1 if deny_on_limit else 0
    q["max_cpus_per_user_raw"] = UNLIMITED_CPU_RAW if max_cpus_per_user is None else int(round(max_cpus_per_user * 256))
    q["max_wall_sec"], q["max_time_limit_per_job_sec"] = max_wall_sec, max_time_limit_per_job_sec
    q["max_tres"] = unlimited_tres() if max_tres is None else max_tres
    q["max_tres_per_user"] = unlimited_tres() if max_tres_per_user is None else max_tres_per_user
    q["max_tres_per_account"] = unlimited_tres() if max_tres_per_account is None else max_tres_per_account
    return q


def submit_part_limit(max_submit_jobs=UNLIMITED_JOBS, max_wall_duration_per_job_sec=abi.SUBMIT_JOB_MAX_TIME_LIMIT_SEC,
                      max_tres_per_job=None) -> np.ndarray:
    p = np.zeros((), SUBMIT_PART_LIMIT_DT)
    p["max_submit_jobs"], p["max_wall_duration_per_job_sec"] = max_submit_jobs, max_wall_duration_per_job_sec
    p["max_tres_per_job"] = unlimited_tres() if max_tres_per_job is None else max_tres_per_job
    return p


@dataclass
class SubmitState:
    """The five submit_jobs_count tables and the three exists arrays (cns_get_submit_usage)."""
    user_qos_submit: np.ndarray
    user_part_submit: np.ndarray
    acct_qos_submit: np.ndarray
    acct_part_submit: np.ndarray
    qos_submit: np.ndarray
    user_exists: np.ndarray
    acct_exists: np.ndarray
    qos_exists: np.ndarray

    def pointers(self):
        return [getattr(self, f).ctypes.data_as(abi._P) for f in self.__dataclass_fields__]

    def same_as(self, o: "SubmitState") -> bool:
        return all(np.array_equal(getattr(self, f), getattr(o, f)) for f in self.__dataclass_fields__)

    def max_count(self) -> int:
        return max([int(getattr(self, f).max()) for f in list(self.__dataclass_fields__)[:5] if len(getattr(self, f))] + [0])


@dataclass
class SubmitTables:
    layout: abi.GresLayout
    num_users: int
    num_user_accts: int
    num_partitions: int
    qos: np.ndarray                        # [Q] SUBMIT_QOS_DT
    acct_parent: np.ndarray                # [A] u32, LIM_NONE for a root
    part_limits: np.ndarray = field(default_factory=lambda: np.zeros(0, SUBMIT_PART_LIMIT_DT))
    user_part_limit: Optional[np.ndarray] = None   # [UA*Pn] u32
    acct_part_limit: Optional[np.ndarray] = None   # [A*Pn] u32
    user_qos: Optional[np.ndarray] = None          # [U*Q] USAGE_DT
    user_part: Optional[np.ndarray] = None         # [UA*Pn]
    acct_qos: Optional[np.ndarray] = None          # [A*Q]
    acct_part: Optional[np.ndarray] = None         # [A*Pn]
    qos_usage: Optional[np.ndarray] = None         # [Q]
    user_qos_submit: Optional[np.ndarray] = None   # u32, shapes as the usage tables
    user_part_submit: Optional[np.ndarray] = None
    acct_qos_submit: Optional[np.ndarray] = None
    acct_part_submit: Optional[np.ndarray] = None
    qos_submit: Optional[np.ndarray] = None
    user_exists: Optional[np.ndarray] = None       # [U] u8
    acct_exists: Optional[np.ndarray] = None       # [A] u8
    qos_exists: Optional[np.ndarray] = None        # [Q] u8

    def __post_init__(self):
        self.qos = np.ascontiguousarray(self.qos, SUBMIT_QOS_DT).reshape(-1)
        self.acct_parent = np.ascontiguousarray(self.acct_parent, np.uint32)
        self.part_limits = np.ascontiguousarray(self.part_limits, SUBMIT_PART_LIMIT_DT).reshape(-1)
        coerce_tables(self)

    @property
    def num_qos(self):
        return len(self.qos)

    @property
    def num_accounts(self):
        return len(self.acct_parent)

    def to_c(self) -> abi.CnsSubmitTables:
        p = lambda a: None if a is None or len(a) == 0 else a.ctypes.data
        s = abi.CnsSubmitTables(self.num_users, self.num_user_accts, self.num_accounts, self.num_qos, self.num_partitions, len(self.part_limits),
                                self.layout.to_c())
        for f, _ in abi.CnsSubmitTables._fields_[7:]:
            setattr(s, f, p(getattr(self, f)))
        return s

    def state(self) -> SubmitState:
        """The counters and exists bits as set (a copy; None = zeros)."""
        sh = table_shapes(self)
        return SubmitState(*[np.zeros(sh[f][1], sh[f][0]) if getattr(self, f) is None else getattr(self, f).copy()
                             for f in SubmitState.__dataclass_fields__])


class SubmitKeys:
    def __init__(self, user, user_acct, account, qos, count=None, skip=None):
        a = lambda x, dt: np.ascontiguousarray(np.asarray(x, dtype=dt))
        self.user, self.user_acct, self.account, self.qos = a(user, np.uint32), a(user_acct, np.uint32), a(account, np.uint32), a(qos, np.uint32)
        self.num_jobs = len(self.user)
        self.count = np.ones(self.num_jobs, np.uint32) if count is None else a(count, np.uint32)
        self.skip = None if skip is None else a(skip, np.uint8)
        for f in ("user_acct", "account", "qos", "count"):
            assert len(getattr(self, f)) == self.num_jobs, f

    def to_c(self) -> abi.CnsSubmitKeys:
        p = lambda x: None if x is None else x.ctypes.data
        return abi.CnsSubmitKeys(p(self.user), p(self.user_acct), p(self.account), p(self.qos), p(self.count), p(self.skip))

    def slice(self, lo, hi) -> "SubmitKeys":
        """Jobs lo..hi, copied."""
        c = lambda a: a[lo:hi].copy()
        return SubmitKeys(c(self.user), c(self.user_acct), c(self.account), c(self.qos), c(self.count), None if self.skip is None else c(self.skip))


def slice_jobs(jobs: abi.Jobs, lo, hi) -> abi.Jobs:
    """Jobs lo..hi of a table, copied (the fields the submit check reads; node lists are not carried over)."""
    g = lambda a: None if a is None else a[lo:hi].copy()
    return abi.Jobs(partition=g(jobs.partition), time_limit_sec=g(jobs.time_limit_sec), node_mem=g(jobs.node_mem),
                    task_cpu_raw=g(jobs.task_cpu_raw), task_mem=g(jobs.task_mem), node_num=g(jobs.node_num), ntasks=g(jobs.ntasks),
                    ntasks_per_node_min=g(jobs.ntasks_per_node_min), ntasks_per_node_max=g(jobs.ntasks_per_node_max),
                    node_cpu_raw=g(jobs.node_cpu_raw), gres_total=g(jobs.gres_total), gres_spec=g(jobs.gres_spec))


__all__ = ["LIM_NONE", "SUBMIT_QOS_DT", "SUBMIT_PART_LIMIT_DT", "SubmitKeys", "SubmitState", "SubmitTables", "slice_jobs", "submit_part_limit",
           "submit_qos"]
