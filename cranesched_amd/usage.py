"""Inputs of the release / charge of the usage tables (include/crane_gpu_usage/usage.h) as numpy tables + ctypes views.

Mirror of what `AccountMetaContainer::DoFreeResource_` / `DoMallocResource_` read and write
(src/CraneCtld/Accounting/AccountMetaContainer.cpp:1067-1208): `UsageTables` = the five MetaResource tables (a cns_usage + its
submit_jobs_count), one exists byte per nested record and per user / account / QoS; `UsageJobs` = one row per Free... / Malloc... call.
Pure plumbing: no arithmetic of the call here.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import abi
from .limits import ENTITIES, LIM_NONE, NESTED, SUBMITS, TABLES, USAGE_DT, coerce_tables, table_shapes


@dataclass
class UsageState:
    """Everything cns_usage_get_tables returns, in the order of cns_usage_tables_out."""
    user_qos: np.ndarray
    user_part: np.ndarray
    acct_qos: np.ndarray
    acct_part: np.ndarray
    qos_usage: np.ndarray
    user_qos_submit: np.ndarray
    user_part_submit: np.ndarray
    acct_qos_submit: np.ndarray
    acct_part_submit: np.ndarray
    qos_submit: np.ndarray
    user_qos_exists: np.ndarray
    user_part_exists: np.ndarray
    acct_qos_exists: np.ndarray
    acct_part_exists: np.ndarray
    user_exists: np.ndarray
    acct_exists: np.ndarray
    qos_exists: np.ndarray

    def pointers(self):
        return [getattr(self, f).ctypes.data if len(getattr(self, f)) else None for f in self.__dataclass_fields__]

    def differences(self, o: "UsageState"):
        """The fields that differ (a usage record is compared without its padding word)."""
        bad = []
        for f in self.__dataclass_fields__:
            a, b = getattr(self, f), getattr(o, f)
            if a.dtype == USAGE_DT:
                same = all(np.array_equal(a[n], b[n]) for n in USAGE_DT.names if n != "reserved0")
            else:
                same = np.array_equal(a, b)
            if not same:
                bad.append(f)
        return bad

    def same_as(self, o: "UsageState") -> bool:
        return not self.differences(o)


@dataclass
class UsageTables:
    layout: abi.GresLayout
    num_users: int
    num_user_accts: int
    num_qos: int
    num_partitions: int
    acct_parent: np.ndarray                        # [A] u32, LIM_NONE for a root
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
    user_qos_exists: Optional[np.ndarray] = None   # u8, shapes as the four nested tables
    user_part_exists: Optional[np.ndarray] = None
    acct_qos_exists: Optional[np.ndarray] = None
    acct_part_exists: Optional[np.ndarray] = None
    user_exists: Optional[np.ndarray] = None       # [U] u8
    acct_exists: Optional[np.ndarray] = None       # [A] u8
    qos_exists: Optional[np.ndarray] = None        # [Q] u8

    def __post_init__(self):
        self.acct_parent = np.ascontiguousarray(self.acct_parent, np.uint32)
        coerce_tables(self)

    @property
    def num_accounts(self):
        return len(self.acct_parent)

    def to_c(self) -> abi.CnsUsageTables:
        p = lambda a: None if a is None or len(a) == 0 else a.ctypes.data
        s = abi.CnsUsageTables(self.num_users, self.num_user_accts, self.num_accounts, self.num_qos, self.num_partitions, 0, self.layout.to_c())
        for f, _ in abi.CnsUsageTables._fields_[7:]:
            setattr(s, f, p(getattr(self, f)))
        return s

    def state(self) -> UsageState:
        """The tables as the engine holds them after cns_usage_set_tables (a copy): None = zeros; a nested exists array that is not given
        = every entry exists if the table or its submit counts are given, none otherwise; a record that does not exist is zero."""
        sh = table_shapes(self)
        v = {f: np.zeros(sh[f][1], sh[f][0]) if getattr(self, f) is None else getattr(self, f).copy() for f in TABLES + SUBMITS + ENTITIES}
        for e, f, s in zip(NESTED, TABLES, SUBMITS):
            given = getattr(self, f) is not None or getattr(self, s) is not None
            ex = getattr(self, e)
            v[e] = np.full(sh[e][1], 1 if given else 0, np.uint8) if ex is None else (ex != 0).astype(np.uint8)
            v[f][v[e] == 0] = np.zeros((), USAGE_DT)
            v[s][v[e] == 0] = 0
        for e in ENTITIES:
            v[e] = (v[e] != 0).astype(np.uint8)
        for f in TABLES:
            v[f]["reserved0"] = 0
        return UsageState(**v)


class UsageJobs:
    """cns_usage_jobs: one row per call of the reference, in call order.  name_total [J, 4], class_count [J, 8]."""

    def __init__(self, user, user_acct, account, qos, partition, cpu_raw=None, mem=None, wall_sec=None, jobs_count=None, submit_count=None,
                 name_total=None, class_count=None, skip=None):
        a = lambda x, dt: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=dt))
        self.user, self.user_acct, self.account, self.qos, self.partition = (a(x, np.uint32) for x in (user, user_acct, account, qos, partition))
        self.num_jobs = len(self.user)
        self.cpu_raw, self.mem, self.wall_sec = a(cpu_raw, np.int64), a(mem, np.uint64), a(wall_sec, np.int64)
        self.jobs_count, self.submit_count, self.skip = a(jobs_count, np.uint32), a(submit_count, np.uint32), a(skip, np.uint8)
        self.name_total = None if name_total is None else a(name_total, np.uint64).reshape(self.num_jobs, abi.MAX_GRES_NAMES)
        self.class_count = None if class_count is None else a(class_count, np.uint64).reshape(self.num_jobs, abi.MAX_GRES_CLASSES)
        for f, _ in abi.CnsUsageJobs._fields_[1:]:
            assert getattr(self, f) is None or len(getattr(self, f)) == self.num_jobs, f

    def to_c(self) -> abi.CnsUsageJobs:
        s = abi.CnsUsageJobs()
        s.num_jobs = self.num_jobs
        for f, _ in abi.CnsUsageJobs._fields_[1:]:
            v = getattr(self, f)
            setattr(s, f, None if v is None or self.num_jobs == 0 else v.ctypes.data)
        return s

    def slice(self, lo, hi) -> "UsageJobs":
        c = lambda x: None if x is None else x[lo:hi].copy()
        return UsageJobs(*[c(getattr(self, f)) for f, _ in abi.CnsUsageJobs._fields_[1:]])

    def take(self, idx) -> "UsageJobs":
        """The rows idx, in that order, copied."""
        c = lambda x: None if x is None else x[np.asarray(idx)].copy()
        return UsageJobs(*[c(getattr(self, f)) for f, _ in abi.CnsUsageJobs._fields_[1:]])


__all__ = ["LIM_NONE", "USAGE_DT", "UsageJobs", "UsageState", "UsageTables"]
