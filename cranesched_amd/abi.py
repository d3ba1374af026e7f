"""ctypes mirror of include/crane_gpu/node_select.h (the C ABI of the engine).

Host-side containers (numpy SoA) for the three tables that cross the boundary of
CraneCtld's `SchedulerAlgo::NodeSelect` (reference: src/CraneCtld/JobScheduler.h:260-263):
the node snapshot (CranedMeta, src/CraneCtld/Node/NodeDefs.h:59-81), the running jobs
(RnJobInScheduler, JobScheduler.h:57-90) and the pending jobs (PdJobInScheduler,
JobScheduler.h:92-170), plus the placement result.  Pure plumbing: no scheduling logic here.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

CNS_ABI_VERSION = 4
RESV_NONE = 0xFFFFFFFF
MAX_GRES_CLASSES = 8
MAX_GRES_NAMES = 4
MAX_NODE_TYPES = 64
NODE_NONE = 0xFFFFFFFF

REASON_NONE, REASON_PRIORITY, REASON_RESOURCE, REASON_RESOURCE_RESERVED, \
    REASON_PARTITION_NOT_FOUND, REASON_SKIPPED, REASON_RESERVATION_NOT_FOUND = range(7)
REASON_ENGINE_REFUSED = 8   # (7: "Preempted", include/crane_gpu/preempt.h)
# cns_partition_status (cns_get_partition_status): why a partition's jobs came back with REASON_ENGINE_REFUSED
PART_SERVED, PART_REFUSED_NODE, PART_REFUSED_CPU, PART_REFUSED_TYPES, PART_REFUSED_WIDTH = range(5)
# cns_reason <-> the reference's reason strings (JobScheduler.cpp:6750-6831, JobScheduler.h:198)
REASON_STR = {
    REASON_NONE: "", REASON_PRIORITY: "Priority", REASON_RESOURCE: "Resource",
    REASON_RESOURCE_RESERVED: "Resource Reserved",
    REASON_PARTITION_NOT_FOUND: "Partition Not Found", REASON_SKIPPED: "<caller-set>",
    REASON_RESERVATION_NOT_FOUND: "Reservation Not Found",
    REASON_ENGINE_REFUSED: "<engine refused the partition: the caller's CPU scheduler takes the job>",
}

STATUS_STR = {0: "CNS_OK", -1: "CNS_ERR_INVALID_ARG", -2: "CNS_ERR_NO_DEVICE", -3: "CNS_ERR_HIP",
              -4: "CNS_ERR_UNSUPPORTED", -5: "CNS_ERR_STATE", -6: "CNS_ERR_DEVICE_FAULT"}


class CnsConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32),
                ("scheduled_batch_size", C.c_uint64), ("max_job_num_per_node", C.c_uint32),
                ("kernel_pin", C.c_uint32), ("max_time_window_sec", C.c_int64)]


class CnsGresLayout(C.Structure):
    _fields_ = [("num_classes", C.c_uint32), ("class_name", C.c_uint8 * MAX_GRES_CLASSES),
                ("class_shift", C.c_uint8 * MAX_GRES_CLASSES),
                ("class_width", C.c_uint8 * MAX_GRES_CLASSES)]


_P = C.c_void_p


class CnsNodeSoa(C.Structure):
    _fields_ = [("num_nodes", C.c_uint32), ("num_partitions", C.c_uint32),
                ("cpu_total_raw", _P), ("mem_total", _P), ("core_lo", _P), ("core_hi", _P),
                ("gres_slots", _P), ("schedulable", _P), ("part_offsets", _P), ("part_nodes", _P),
                ("gres", CnsGresLayout), ("core_w2", _P), ("core_w3", _P), ("unsupported", _P)]


class CnsRunningSoa(C.Structure):
    _fields_ = [("num_jobs", C.c_uint32), ("num_allocs", C.c_uint32), ("end_sec", _P),
                ("alloc_offsets", _P), ("alloc_node", _P), ("alloc_cpu_raw", _P), ("alloc_mem", _P),
                ("alloc_core_lo", _P), ("alloc_core_hi", _P), ("alloc_gres", _P), ("reservation", _P),
                ("alloc_core_w2", _P), ("alloc_core_w3", _P)]


class CnsResvSoa(C.Structure):
    _fields_ = [("num_resv", C.c_uint32), ("num_allocs", C.c_uint32), ("start_sec", _P), ("end_sec", _P),
                ("alloc_offsets", _P), ("alloc_node", _P), ("alloc_cpu_raw", _P), ("alloc_mem", _P),
                ("alloc_core_lo", _P), ("alloc_core_hi", _P), ("alloc_gres", _P), ("alloc_core_w2", _P), ("alloc_core_w3", _P)]


class CnsJobSoa(C.Structure):
    _fields_ = [("num_jobs", C.c_uint64), ("partition", _P), ("time_limit_sec", _P),
                ("node_cpu_raw", _P), ("node_mem", _P), ("task_cpu_raw", _P), ("task_mem", _P),
                ("node_num", _P), ("ntasks", _P), ("ntasks_per_node_min", _P),
                ("ntasks_per_node_max", _P), ("exclusive", _P), ("gres_total", _P),
                ("gres_spec", _P), ("incl_offsets", _P), ("incl_nodes", _P), ("excl_offsets", _P),
                ("excl_nodes", _P), ("skip", _P), ("reservation", _P)]


class CnsPlacementSoa(C.Structure):
    _fields_ = [("place_capacity", C.c_uint64), ("start_sec", _P), ("reason", _P),
                ("place_offsets", _P), ("node_idx", _P), ("ntasks", _P), ("cpu_raw", _P),
                ("mem", _P), ("core_lo", _P), ("core_hi", _P), ("gres", _P), ("core_w2", _P), ("core_w3", _P)]


class CnsTiming(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("init_ms", C.c_double), ("select_ms", C.c_double),
                ("d2h_ms", C.c_double), ("jobs_ordered", C.c_uint64),
                ("algorithmic_bytes", C.c_uint64)]


class CnsResultsOffsets(C.Structure):   # cns_results_offsets
    _fields_ = [("num_jobs", C.c_uint64), ("num_places", C.c_uint64), ("wide_cores", C.c_uint32), ("reserved0", C.c_uint32)] + \
               [(f, C.c_uint64) for f in ("start_sec", "cpu_raw", "mem", "core_lo", "core_hi", "gres", "node_idx", "ntasks", "reason",
                                          "core_w2", "core_w3", "total_bytes")]


class CnsGroupInfo(C.Structure):        # cns_group_info
    _fields_ = [("num_devices", C.c_uint32), ("gather_mode", C.c_uint32), ("shards_ms", C.c_double), ("max_select_ms", C.c_double),
                ("allgather_ms", C.c_double), ("download_ms", C.c_double), ("scatter_ms", C.c_double), ("slot_bytes", C.c_uint64)]


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_P)


def _arr(x, dtype, n=None):
    a = np.ascontiguousarray(x, dtype=dtype)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"expected leading dim {n}, got {a.shape}")
    return a


@dataclass
class GresLayout:
    """(name,type) classes of the 64-bit GRES slot mask."""
    class_name: list = field(default_factory=list)   # name-group id per class
    class_shift: list = field(default_factory=list)
    class_width: list = field(default_factory=list)

    def to_c(self) -> CnsGresLayout:
        g = CnsGresLayout()
        g.num_classes = len(self.class_name)
        for i, (a, s, w) in enumerate(zip(self.class_name, self.class_shift, self.class_width)):
            g.class_name[i], g.class_shift[i], g.class_width[i] = a, s, w
        return g

    def class_mask(self, g: int) -> int:
        return ((1 << self.class_width[g]) - 1) << self.class_shift[g]


@dataclass
class Cluster:
    """Per-cycle node snapshot (cns_node_soa)."""
    cpu_total_raw: np.ndarray
    mem_total: np.ndarray
    core_lo: np.ndarray
    core_hi: np.ndarray
    gres_slots: np.ndarray
    part_offsets: np.ndarray
    part_nodes: np.ndarray
    gres: GresLayout = field(default_factory=GresLayout)
    schedulable: Optional[np.ndarray] = None
    core_w2: Optional[np.ndarray] = None    # core ids 128..191 / 192..255 (ABI 3); None = no node has any
    core_w3: Optional[np.ndarray] = None
    unsupported: Optional[np.ndarray] = None   # [N] uint8 (ABI 4): nodes the caller could not express (core id >= 256, too many GRES slots); None = none

    def __post_init__(self):
        n = len(self.cpu_total_raw)
        if self.unsupported is not None:
            self.unsupported = _arr(self.unsupported, np.uint8, n)
        if self.core_w2 is not None:
            self.core_w2 = _arr(self.core_w2, np.uint64, n)
        if self.core_w3 is not None:
            self.core_w3 = _arr(self.core_w3, np.uint64, n)
        self.cpu_total_raw = _arr(self.cpu_total_raw, np.int64)
        self.mem_total = _arr(self.mem_total, np.uint64, n)
        self.core_lo = _arr(self.core_lo, np.uint64, n)
        self.core_hi = _arr(self.core_hi, np.uint64, n)
        self.gres_slots = _arr(self.gres_slots, np.uint64, n)
        self.part_offsets = _arr(self.part_offsets, np.uint32)
        self.part_nodes = _arr(self.part_nodes, np.uint32)
        if self.schedulable is not None:
            self.schedulable = _arr(self.schedulable, np.uint8, n)

    @property
    def num_nodes(self):
        return len(self.cpu_total_raw)

    @property
    def num_partitions(self):
        return len(self.part_offsets) - 1

    @property
    def wide_cores(self) -> bool:
        """A node has a core id above 127: results carry the core_w2 / core_w3 planes (cns_placement_soa, packed buffer)."""
        return bool((self.core_w2 is not None and self.core_w2.any()) or (self.core_w3 is not None and self.core_w3.any()))

    def to_c(self) -> CnsNodeSoa:
        s = CnsNodeSoa()
        s.num_nodes, s.num_partitions = self.num_nodes, self.num_partitions
        s.cpu_total_raw, s.mem_total = _ptr(self.cpu_total_raw), _ptr(self.mem_total)
        s.core_lo, s.core_hi, s.gres_slots = _ptr(self.core_lo), _ptr(self.core_hi), _ptr(self.gres_slots)
        s.schedulable = _ptr(self.schedulable)
        s.part_offsets, s.part_nodes = _ptr(self.part_offsets), _ptr(self.part_nodes)
        s.gres = self.gres.to_c()
        s.core_w2, s.core_w3 = _ptr(self.core_w2), _ptr(self.core_w3)
        s.unsupported = _ptr(self.unsupported)
        return s


@dataclass
class Running:
    """Running jobs' allocations (cns_running_soa)."""
    end_sec: np.ndarray
    alloc_offsets: np.ndarray
    alloc_node: np.ndarray
    alloc_cpu_raw: np.ndarray
    alloc_mem: np.ndarray
    alloc_core_lo: np.ndarray
    alloc_core_hi: np.ndarray
    alloc_gres: np.ndarray
    reservation: Optional[np.ndarray] = None   # [R] reservation index or RESV_NONE
    alloc_core_w2: Optional[np.ndarray] = None
    alloc_core_w3: Optional[np.ndarray] = None

    def __post_init__(self):
        self.end_sec = _arr(self.end_sec, np.int64)
        if self.reservation is not None:
            self.reservation = _arr(self.reservation, np.uint32, len(self.end_sec))
        self.alloc_offsets = _arr(self.alloc_offsets, np.uint32, len(self.end_sec) + 1)
        m = int(self.alloc_offsets[-1]) if len(self.alloc_offsets) else 0
        self.alloc_node = _arr(self.alloc_node, np.uint32, m)
        self.alloc_cpu_raw = _arr(self.alloc_cpu_raw, np.int64, m)
        self.alloc_mem = _arr(self.alloc_mem, np.uint64, m)
        self.alloc_core_lo = _arr(self.alloc_core_lo, np.uint64, m)
        self.alloc_core_hi = _arr(self.alloc_core_hi, np.uint64, m)
        self.alloc_gres = _arr(self.alloc_gres, np.uint64, m)
        if self.alloc_core_w2 is not None:
            self.alloc_core_w2 = _arr(self.alloc_core_w2, np.uint64, m)
        if self.alloc_core_w3 is not None:
            self.alloc_core_w3 = _arr(self.alloc_core_w3, np.uint64, m)

    def to_c(self) -> CnsRunningSoa:
        s = CnsRunningSoa()
        s.num_jobs, s.num_allocs = len(self.end_sec), len(self.alloc_node)
        s.end_sec, s.alloc_offsets, s.alloc_node = _ptr(self.end_sec), _ptr(self.alloc_offsets), _ptr(self.alloc_node)
        s.alloc_cpu_raw, s.alloc_mem = _ptr(self.alloc_cpu_raw), _ptr(self.alloc_mem)
        s.alloc_core_lo, s.alloc_core_hi, s.alloc_gres = _ptr(self.alloc_core_lo), _ptr(self.alloc_core_hi), _ptr(self.alloc_gres)
        s.reservation = _ptr(self.reservation)
        s.alloc_core_w2, s.alloc_core_w3 = _ptr(self.alloc_core_w2), _ptr(self.alloc_core_w3)
        return s


@dataclass
class Reservations:
    """Reservations of the cycle (cns_resv_soa): start / end and the reserved resources per node."""
    start_sec: np.ndarray
    end_sec: np.ndarray
    alloc_offsets: np.ndarray
    alloc_node: np.ndarray
    alloc_cpu_raw: np.ndarray
    alloc_mem: np.ndarray
    alloc_core_lo: np.ndarray
    alloc_core_hi: np.ndarray
    alloc_gres: np.ndarray
    alloc_core_w2: Optional[np.ndarray] = None
    alloc_core_w3: Optional[np.ndarray] = None

    def __post_init__(self):
        self.start_sec = _arr(self.start_sec, np.int64)
        v = len(self.start_sec)
        self.end_sec = _arr(self.end_sec, np.int64, v)
        self.alloc_offsets = _arr(self.alloc_offsets, np.uint32, v + 1)
        m = int(self.alloc_offsets[-1]) if len(self.alloc_offsets) else 0
        self.alloc_node = _arr(self.alloc_node, np.uint32, m)
        self.alloc_cpu_raw = _arr(self.alloc_cpu_raw, np.int64, m)
        self.alloc_mem = _arr(self.alloc_mem, np.uint64, m)
        self.alloc_core_lo = _arr(self.alloc_core_lo, np.uint64, m)
        self.alloc_core_hi = _arr(self.alloc_core_hi, np.uint64, m)
        self.alloc_gres = _arr(self.alloc_gres, np.uint64, m)
        if self.alloc_core_w2 is not None:
            self.alloc_core_w2 = _arr(self.alloc_core_w2, np.uint64, m)
        if self.alloc_core_w3 is not None:
            self.alloc_core_w3 = _arr(self.alloc_core_w3, np.uint64, m)

    @property
    def num_resv(self):
        return len(self.start_sec)

    def to_c(self) -> CnsResvSoa:
        s = CnsResvSoa()
        s.num_resv, s.num_allocs = len(self.start_sec), len(self.alloc_node)
        s.start_sec, s.end_sec, s.alloc_offsets = _ptr(self.start_sec), _ptr(self.end_sec), _ptr(self.alloc_offsets)
        s.alloc_node, s.alloc_cpu_raw, s.alloc_mem = _ptr(self.alloc_node), _ptr(self.alloc_cpu_raw), _ptr(self.alloc_mem)
        s.alloc_core_lo, s.alloc_core_hi, s.alloc_gres = _ptr(self.alloc_core_lo), _ptr(self.alloc_core_hi), _ptr(self.alloc_gres)
        s.alloc_core_w2, s.alloc_core_w3 = _ptr(self.alloc_core_w2), _ptr(self.alloc_core_w3)
        return s


@dataclass
class Jobs:
    """Pending jobs in priority order (cns_job_soa)."""
    partition: np.ndarray
    time_limit_sec: np.ndarray
    node_mem: np.ndarray
    task_cpu_raw: np.ndarray
    task_mem: np.ndarray
    node_num: np.ndarray
    ntasks: np.ndarray
    ntasks_per_node_min: np.ndarray
    ntasks_per_node_max: np.ndarray
    node_cpu_raw: Optional[np.ndarray] = None
    exclusive: Optional[np.ndarray] = None
    gres_total: Optional[np.ndarray] = None   # [J, 4] uint8
    gres_spec: Optional[np.ndarray] = None    # [J, 8] uint8
    incl_offsets: Optional[np.ndarray] = None
    incl_nodes: Optional[np.ndarray] = None
    excl_offsets: Optional[np.ndarray] = None
    excl_nodes: Optional[np.ndarray] = None
    skip: Optional[np.ndarray] = None
    reservation: Optional[np.ndarray] = None   # [J] reservation index or RESV_NONE

    def __post_init__(self):
        j = len(self.partition)
        if self.reservation is not None:
            self.reservation = _arr(self.reservation, np.uint32, j)
        self.partition = _arr(self.partition, np.uint32)
        self.time_limit_sec = _arr(self.time_limit_sec, np.int64, j)
        self.node_mem = _arr(self.node_mem, np.uint64, j)
        self.task_cpu_raw = _arr(self.task_cpu_raw, np.int64, j)
        self.task_mem = _arr(self.task_mem, np.uint64, j)
        self.node_num = _arr(self.node_num, np.uint32, j)
        self.ntasks = _arr(self.ntasks, np.uint32, j)
        self.ntasks_per_node_min = _arr(self.ntasks_per_node_min, np.uint32, j)
        self.ntasks_per_node_max = _arr(self.ntasks_per_node_max, np.uint32, j)
        for name, dt in (("node_cpu_raw", np.int64), ("exclusive", np.uint8), ("skip", np.uint8)):
            v = getattr(self, name)
            if v is not None:
                setattr(self, name, _arr(v, dt, j))
        if self.gres_total is not None:
            self.gres_total = _arr(self.gres_total, np.uint8, j).reshape(j, MAX_GRES_NAMES)
        if self.gres_spec is not None:
            self.gres_spec = _arr(self.gres_spec, np.uint8, j).reshape(j, MAX_GRES_CLASSES)
        for off, lst in (("incl_offsets", "incl_nodes"), ("excl_offsets", "excl_nodes")):
            if getattr(self, off) is not None:
                setattr(self, off, _arr(getattr(self, off), np.uint64, j + 1))
                setattr(self, lst, _arr(getattr(self, lst), np.uint32))

    @property
    def num_jobs(self):
        return len(self.partition)

    def total_places(self) -> int:
        return int(self.node_num.astype(np.uint64).sum())

    def to_c(self) -> CnsJobSoa:
        s = CnsJobSoa()
        s.num_jobs = self.num_jobs
        for f, _ in CnsJobSoa._fields_[1:]:
            setattr(s, f, _ptr(getattr(self, f)))
        return s


class Placements:
    """Caller-allocated result arrays (cns_placement_soa)."""

    def __init__(self, num_jobs: int, capacity: int, alloc=None):
        """alloc(n, dtype, fill) -> array: where the arrays live (default: numpy; GpuNodeSelector.pinned: page-locked memory)."""
        self.num_jobs, self.capacity = num_jobs, capacity
        cap = max(capacity, 1)
        if alloc is None:
            alloc = lambda n, dt, fill=0: np.full(n, fill, dt) if fill else np.zeros(n, dt)
        self.start_sec = alloc(max(num_jobs, 1), np.int64, 0)
        self.reason = alloc(max(num_jobs, 1), np.uint8, 0)
        self.place_offsets = alloc(num_jobs + 1, np.uint64, 0)
        self.node_idx = alloc(cap, np.uint32, NODE_NONE)
        self.ntasks = alloc(cap, np.uint32, 0)
        self.cpu_raw = alloc(cap, np.int64, 0)
        self.mem = alloc(cap, np.uint64, 0)
        self.core_lo = alloc(cap, np.uint64, 0)
        self.core_hi = alloc(cap, np.uint64, 0)
        self.gres = alloc(cap, np.uint64, 0)
        self.core_w2 = alloc(cap, np.uint64, 0)
        self.core_w3 = alloc(cap, np.uint64, 0)

    def to_c(self) -> CnsPlacementSoa:
        s = CnsPlacementSoa()
        s.place_capacity = self.capacity
        for f, _ in CnsPlacementSoa._fields_[1:]:
            setattr(s, f, _ptr(getattr(self, f)))
        return s

    FIELDS = ("start_sec", "reason", "place_offsets", "node_idx", "ntasks", "cpu_raw", "mem",
              "core_lo", "core_hi", "gres", "core_w2", "core_w3")

    def trimmed(self):
        """Dict of result arrays cut to their logical lengths (for comparisons / hashing)."""
        j, c = self.num_jobs, self.capacity
        return {"start_sec": self.start_sec[:j], "reason": self.reason[:j],
                "place_offsets": self.place_offsets[:j + 1], "node_idx": self.node_idx[:c],
                "ntasks": self.ntasks[:c], "cpu_raw": self.cpu_raw[:c], "mem": self.mem[:c],
                "core_lo": self.core_lo[:c], "core_hi": self.core_hi[:c], "gres": self.gres[:c],
                "core_w2": self.core_w2[:c], "core_w3": self.core_w3[:c]}

    def diff(self, other: "Placements"):
        """First differing (field, index) between two results, or None if bit-identical."""
        a, b = self.trimmed(), other.trimmed()
        for k in self.FIELDS:
            if a[k].shape != b[k].shape:
                return (k, "shape", a[k].shape, b[k].shape)
            ne = np.nonzero(a[k] != b[k])[0]
            if len(ne):
                i = int(ne[0])
                return (k, i, a[k][i].item(), b[k][i].item(), f"{len(ne)} mismatches")
        return None


# ---------------------------------------------------------------------------------------------------------
# include/crane_gpu/preempt.h
# ---------------------------------------------------------------------------------------------------------
REASON_PREEMPTED = 7
PREEMPT_REF_PENDING = 0x80000000


class CnsPreemptSoa(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("num_qos", C.c_uint32), ("qos_preempt_offsets", C.c_void_p),
                ("qos_preempt", C.c_void_p), ("pd_job_id", C.c_void_p), ("pd_qos", C.c_void_p),
                ("pd_qos_priority", C.c_void_p), ("pd_priority", C.c_void_p), ("rn_job_id", C.c_void_p),
                ("rn_qos", C.c_void_p), ("rn_qos_priority", C.c_void_p), ("rn_start_sec", C.c_void_p),
                ("num_preempting", C.c_uint32), ("reserved0", C.c_uint32), ("preempting_job_ids", C.c_void_p)]


class CnsPreemptOut(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("offsets", C.c_void_p), ("preempted", C.c_void_p),
                ("cancel_capacity", C.c_uint32), ("num_cancelled", C.c_uint32), ("cancelled_job_ids", C.c_void_p),
                ("preempting_capacity", C.c_uint32), ("num_preempting", C.c_uint32), ("preempting_job_ids", C.c_void_p)]


@dataclass
class Preempt:
    """Preemption inputs of one cycle (cns_preempt_soa): QoS preempt lists, the fields TryPreempt_ reads of the pending
    and running jobs, and m_preempting_set_ as the previous cycle left it."""
    qos_preempt: list                      # qos id -> list of qos ids it may preempt
    pd_job_id: np.ndarray
    pd_qos: np.ndarray
    pd_qos_priority: np.ndarray
    pd_priority: np.ndarray
    rn_job_id: np.ndarray
    rn_qos: np.ndarray
    rn_qos_priority: np.ndarray
    rn_start_sec: np.ndarray
    preempting: np.ndarray = None
    enabled: bool = True

    def __post_init__(self):
        self.pd_job_id = _arr(self.pd_job_id, np.uint32); n = len(self.pd_job_id)
        self.pd_qos = _arr(self.pd_qos, np.uint32, n)
        self.pd_qos_priority = _arr(self.pd_qos_priority, np.uint32, n)
        self.pd_priority = _arr(self.pd_priority, np.float64, n)
        self.rn_job_id = _arr(self.rn_job_id, np.uint32); r = len(self.rn_job_id)
        self.rn_qos = _arr(self.rn_qos, np.uint32, r)
        self.rn_qos_priority = _arr(self.rn_qos_priority, np.uint32, r)
        self.rn_start_sec = _arr(self.rn_start_sec, np.int64, r)
        self.preempting = _arr(self.preempting if self.preempting is not None else [], np.uint32)
        off = [0]
        flat = []
        for lst in self.qos_preempt:
            flat.extend(int(x) for x in lst)
            off.append(len(flat))
        self._off = np.asarray(off, np.uint32)
        self._flat = np.asarray(flat if flat else [0], np.uint32)

    def to_c(self) -> CnsPreemptSoa:
        s = CnsPreemptSoa()
        s.enabled, s.num_qos = int(self.enabled), len(self.qos_preempt)
        s.qos_preempt_offsets, s.qos_preempt = _ptr(self._off), _ptr(self._flat)
        for f in ("pd_job_id", "pd_qos", "pd_qos_priority", "pd_priority", "rn_job_id", "rn_qos", "rn_qos_priority", "rn_start_sec"):
            setattr(s, f, _ptr(getattr(self, f)))
        s.num_preempting, s.preempting_job_ids = len(self.preempting), _ptr(self.preempting if len(self.preempting) else np.zeros(1, np.uint32))
        return s


class PreemptOut:
    """Caller-allocated preemption results (cns_preempt_out)."""

    def __init__(self, num_jobs: int, num_running: int, capacity: int = 0):
        self.num_jobs = num_jobs
        cap = max(capacity or (num_jobs + num_running) * 4, 1)
        self.capacity = cap
        self.offsets = np.zeros(num_jobs + 1, np.uint64)
        self.preempted = np.zeros(cap, np.uint32)
        self.cancelled = np.zeros(max(num_running, 1), np.uint32)
        self.preempting = np.zeros(max(2 * num_running, 1), np.uint32)
        self._c = None

    def to_c(self) -> CnsPreemptOut:
        s = CnsPreemptOut()
        s.capacity, s.offsets, s.preempted = self.capacity, _ptr(self.offsets), _ptr(self.preempted)
        s.cancel_capacity, s.cancelled_job_ids = len(self.cancelled), _ptr(self.cancelled)
        s.preempting_capacity, s.preempting_job_ids = len(self.preempting), _ptr(self.preempting)
        self._c = s
        return s

    def lists(self):
        """[(is_pending, index), ...] per pending job."""
        out = []
        for j in range(self.num_jobs):
            refs = self.preempted[int(self.offsets[j]):int(self.offsets[j + 1])]
            out.append([(bool(r & PREEMPT_REF_PENDING), int(r & 0x7FFFFFFF)) for r in refs])
        return out

    def cancelled_ids(self):
        return [int(x) for x in self.cancelled[:self._c.num_cancelled]]

    def preempting_ids(self):
        return [int(x) for x in self.preempting[:self._c.num_preempting]]


# ---- reservation what-ifs (include/crane_gpu_resv/resv_probe.h) ---------------------------------------------------------
RESVQ_OK, RESVQ_NOT_ENOUGH, RESVQ_IN_THE_PAST = 0, 1, 2
RESVQ_FREE, RESVQ_RUNNING, RESVQ_RESERVED, RESVQ_NOT_FOUND = 0, 1, 2, 3
# cns_resvq_shape's arguments, in the header's order
ResvqShape = namedtuple("ResvqShape", ("pick_block", "pick_grid", "sort_tile", "scan_span"))
# cns_preempt_shape's arguments (include/crane_gpu/preempt.h), in the header's order
PreemptShape = namedtuple("PreemptShape", ("sort_lanes", "rank_sort_max", "compact_records", "cache_nodes", "pool_nodes"))


# cns_select_shape (include/crane_gpu/node_select.h): the constants at which the selection kernels change path
SHAPE_MAX_WIDTHS = 8


class CnsTileShape(C.Structure):
    _fields_ = [("lanes", C.c_uint32), ("num_widths", C.c_uint32), ("widths", C.c_uint32 * SHAPE_MAX_WIDTHS)]


class CnsSelectShapeInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("tl_chunk", "tl_cap", "multi_k", "pipe_max_k", "max_upd", "lds_heap", "alloc_cache", "pipe_ring",
                                          "wide_task_ring", "pipe_xring", "wide_window", "sel_dip_max_npl")] + \
               [("select", CnsTileShape), ("pipe", CnsTileShape), ("wide", CnsTileShape * 4), ("wide_waves", C.c_uint32 * 4)]


TileShape = namedtuple("TileShape", ("lanes", "widths"))          # widths: ascending tuple of rows per lane
# the scalar fields in the header's order, then select / pipe (TileShape) and wide: a tuple of (scanner waves, TileShape), widest build first
SelectShape = namedtuple("SelectShape", tuple(f for f, t in CnsSelectShapeInfo._fields_ if t is C.c_uint32) + ("select", "pipe", "wide"))


# cns_serial_shape (include/crane_gpu/node_select.h): the loop shapes of the serial protocol (k_mem, k_giant)
class CnsSerialShapeInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("scan_lanes", "scan_trip_rows", "mem_words", "giant_mem_words", "mem_slots", "giant_mem_slots", "helper_lanes",
                                          "helper_trip_slots", "helpers_max", "helper_budget", "helpers_min", "select_tile_slots")]


SerialShape = namedtuple("SerialShape", tuple(f for f, _ in CnsSerialShapeInfo._fields_))


# cns_probe_shape (include/crane_gpu_probe/probe.h): the constants at which k_probe changes path
class CnsProbeShapeInfo(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("block", "dip_cpu_sat", "dip_mem_sat", "dip_gres_sat", "gres_classes", "gres_names", "max_types",
                                          "heap_ent_bytes", "loff_clamp", "pad")] + [("scratch_cap", C.c_uint64)]


ProbeShape = namedtuple("ProbeShape", tuple(f for f, _ in CnsProbeShapeInfo._fields_ if f != "pad"))


class CnsResvqSoa(C.Structure):
    _fields_ = [("num_queries", C.c_uint64), ("start_sec", _P), ("duration_sec", _P), ("node_num", _P), ("cand_offsets", _P),
                ("cand_nodes", _P), ("find_earliest", _P)]


class CnsResvqOut(C.Structure):
    _fields_ = [("code_capacity", C.c_uint64), ("chosen_capacity", C.c_uint64), ("status", _P), ("start_sec", _P), ("num_free", _P),
                ("code", _P), ("chosen_offsets", _P), ("chosen_nodes", _P)]


@dataclass
class ResvQueries:
    """Q reservation requests (cns_resvq_soa): start, duration, node count (0: the whole list), candidates in the caller's order."""
    start_sec: np.ndarray
    duration_sec: np.ndarray
    node_num: np.ndarray
    cand_offsets: np.ndarray
    cand_nodes: np.ndarray
    find_earliest: Optional[np.ndarray] = None

    def __post_init__(self):
        self.start_sec = _arr(self.start_sec, np.int64)
        q = len(self.start_sec)
        self.duration_sec = _arr(self.duration_sec, np.int64, q)
        self.node_num = _arr(self.node_num, np.uint32, q)
        self.cand_offsets = _arr(self.cand_offsets, np.uint64, q + 1)
        self.cand_nodes = _arr(self.cand_nodes, np.uint32)
        if self.find_earliest is not None:
            self.find_earliest = _arr(self.find_earliest, np.uint8, q)

    @property
    def num_queries(self):
        return len(self.start_sec)

    def k(self) -> np.ndarray:
        """Nodes asked for per query: node_num, or the list length (JobScheduler.cpp:4357-4358)."""
        lens = np.diff(self.cand_offsets.astype(np.int64))
        return np.where(self.node_num != 0, self.node_num.astype(np.int64), lens)

    def take(self, order) -> "ResvQueries":
        """The queries `order`, in that order."""
        order = np.asarray(order, np.int64)
        lens = np.diff(self.cand_offsets.astype(np.int64))[order]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        parts = [self.cand_nodes[int(self.cand_offsets[i]):int(self.cand_offsets[i + 1])] for i in order]
        nodes = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
        return ResvQueries(self.start_sec[order], self.duration_sec[order], self.node_num[order], off, nodes,
                           None if self.find_earliest is None else self.find_earliest[order])

    def to_c(self) -> CnsResvqSoa:
        s = CnsResvqSoa()
        s.num_queries = self.num_queries
        s.start_sec, s.duration_sec, s.node_num = _ptr(self.start_sec), _ptr(self.duration_sec), _ptr(self.node_num)
        s.cand_offsets, s.cand_nodes, s.find_earliest = _ptr(self.cand_offsets), _ptr(self.cand_nodes), _ptr(self.find_earliest)
        return s


class ResvAnswers:
    """Caller-allocated cns_resvq_out: status / start_sec / num_free per query, code per candidate, the chosen nodes as a CSR."""
    FIELDS = ("status", "start_sec", "num_free", "code", "chosen_offsets", "chosen_nodes")

    def __init__(self, queries: "ResvQueries", code_capacity: int | None = None, chosen_capacity: int | None = None):
        q = queries.num_queries
        lens = np.diff(queries.cand_offsets.astype(np.int64))
        self.num_queries = q
        self.code_capacity = int(lens.sum()) if code_capacity is None else code_capacity
        self.chosen_capacity = int(np.minimum(queries.k(), lens).sum()) if chosen_capacity is None else chosen_capacity
        self.status = np.zeros(max(q, 1), np.uint8)
        self.start_sec = np.zeros(max(q, 1), np.int64)
        self.num_free = np.zeros(max(q, 1), np.uint32)
        self.code = np.zeros(max(self.code_capacity, 1), np.uint8)
        self.chosen_offsets = np.zeros(q + 1, np.uint64)
        self.chosen_nodes = np.zeros(max(self.chosen_capacity, 1), np.uint32)
        self._codes = int(lens.sum())

    def to_c(self) -> CnsResvqOut:
        s = CnsResvqOut()
        s.code_capacity, s.chosen_capacity = self.code_capacity, self.chosen_capacity
        s.status, s.start_sec, s.num_free, s.code = _ptr(self.status), _ptr(self.start_sec), _ptr(self.num_free), _ptr(self.code)
        s.chosen_offsets, s.chosen_nodes = _ptr(self.chosen_offsets), _ptr(self.chosen_nodes)
        return s

    def trimmed(self) -> dict:
        """The arrays cut to what the call wrote."""
        q = self.num_queries
        return {"status": self.status[:q], "start_sec": self.start_sec[:q], "num_free": self.num_free[:q], "code": self.code[:self._codes],
                "chosen_offsets": self.chosen_offsets, "chosen_nodes": self.chosen_nodes[:int(self.chosen_offsets[q])]}


# ---- validity of a batch of submissions (include/crane_gpu_valid/validity.h) ---------------------------------------------
(VALID_OK, VALID_BAD_REQUEST, VALID_ZERO_MEM, VALID_ZERO_CPU, VALID_PARTITION_NOT_FOUND, VALID_REFUSED, VALID_NO_RESOURCE,
 VALID_NODE_NUM, VALID_RESV_NOT_FOUND, VALID_RESV_NODE, VALID_NOT_ENOUGH_NODES) = range(11)
VALID_STR = {VALID_OK: "OK", VALID_BAD_REQUEST: "BAD_REQUEST", VALID_ZERO_MEM: "ZERO_MEM", VALID_ZERO_CPU: "ZERO_CPU",
             VALID_PARTITION_NOT_FOUND: "PARTITION_NOT_FOUND", VALID_REFUSED: "REFUSED", VALID_NO_RESOURCE: "NO_RESOURCE",
             VALID_NODE_NUM: "NODE_NUM", VALID_RESV_NOT_FOUND: "RESV_NOT_FOUND", VALID_RESV_NODE: "RESV_NODE",
             VALID_NOT_ENOUGH_NODES: "NOT_ENOUGH_NODES"}


class CnsValidityOut(C.Structure):
    _fields_ = [("code", _P), ("eligible", _P)]


# ---- the commit loop's checks behind a cycle (include/crane_gpu_commit/commit_check.h) ------------------------------------
CC_TIME_INFINITE_PAST = -(1 << 63)
(COMMIT_OK, COMMIT_GONE, COMMIT_NOT_STARTED, COMMIT_RESOURCE_CHANGED, COMMIT_RESV_DELETED, COMMIT_RESV_ENDS_EARLY, COMMIT_RESV_CHANGED,
 COMMIT_WAITING_PREEMPTION) = range(8)
COMMIT_STR = {COMMIT_OK: "OK", COMMIT_GONE: "GONE", COMMIT_NOT_STARTED: "NOT_STARTED", COMMIT_RESOURCE_CHANGED: "RESOURCE_CHANGED",
              COMMIT_RESV_DELETED: "RESV_DELETED", COMMIT_RESV_ENDS_EARLY: "RESV_ENDS_EARLY", COMMIT_RESV_CHANGED: "RESV_CHANGED",
              COMMIT_WAITING_PREEMPTION: "WAITING_PREEMPTION"}
# what the reference writes into job->reason there (JobScheduler.cpp:1518-1552); "" where it writes nothing
COMMIT_REASON = {COMMIT_OK: "", COMMIT_GONE: "", COMMIT_NOT_STARTED: "", COMMIT_RESOURCE_CHANGED: "Resource changed",
                 COMMIT_RESV_DELETED: "Reservation deleted", COMMIT_RESV_ENDS_EARLY: "Resource", COMMIT_RESV_CHANGED: "Reservation changed",
                 COMMIT_WAITING_PREEMPTION: "Waiting for Preemption"}


class CnsCommitEvents(C.Structure):
    _fields_ = [("num_node_events", C.c_uint32), ("num_affected_resv", C.c_uint32), ("ev_time_sec", _P), ("ev_offsets", _P), ("ev_nodes", _P),
                ("ar_resv", _P), ("ar_exists", _P), ("ar_end_sec", _P), ("ar_offsets", _P), ("ar_nodes", _P)]


class CnsCommitJobs(C.Structure):
    _fields_ = [("num_jobs", C.c_uint64), ("time_limit_sec", _P), ("reservation", _P), ("gone", _P), ("preempt_offsets", _P), ("preempted", _P),
                ("num_running", C.c_uint32), ("reserved0", C.c_uint32), ("running_alive", _P)]


class CnsCommitOut(C.Structure):
    _fields_ = [("code", _P), ("counts", _P)]


# ---- the pending gate in front of a cycle (include/crane_gpu_gate/pending_gate.h) ----------------------------------------
GATE_TIME_INFINITE_FUTURE = (1 << 63) - 1
GATE_TIME_INFINITE_PAST = -(1 << 63)
(GATE_OK, GATE_OK_ARRAY_PARENT, GATE_HELD, GATE_BEGIN_TIME, GATE_DEPENDENCY, GATE_DEPENDENCY_NEVER, GATE_ARRAY_NO_META, GATE_ARRAY_COMPLETE,
 GATE_ARRAY_CANCELLED, GATE_ARRAY_DEADLINE, GATE_ARRAY_NO_NEXT, GATE_ARRAY_TASK_LIMIT) = range(12)
GATE_STR = {GATE_OK: "OK", GATE_OK_ARRAY_PARENT: "OK_ARRAY_PARENT", GATE_HELD: "HELD", GATE_BEGIN_TIME: "BEGIN_TIME", GATE_DEPENDENCY: "DEPENDENCY",
            GATE_DEPENDENCY_NEVER: "DEPENDENCY_NEVER", GATE_ARRAY_NO_META: "ARRAY_NO_META", GATE_ARRAY_COMPLETE: "ARRAY_COMPLETE",
            GATE_ARRAY_CANCELLED: "ARRAY_CANCELLED", GATE_ARRAY_DEADLINE: "ARRAY_DEADLINE", GATE_ARRAY_NO_NEXT: "ARRAY_NO_NEXT",
            GATE_ARRAY_TASK_LIMIT: "ARRAY_TASK_LIMIT"}
# what the reference writes into job->pending_reason there (JobScheduler.cpp:1381-1392, Array.cpp:238-256); "" where it writes ""
GATE_REASON = {GATE_OK: "", GATE_OK_ARRAY_PARENT: "", GATE_HELD: "Held", GATE_BEGIN_TIME: "BeginTime", GATE_DEPENDENCY: "Dependency",
               GATE_DEPENDENCY_NEVER: "DependencyNeverSatisfied", GATE_ARRAY_NO_META: "", GATE_ARRAY_COMPLETE: "ArrayMaterializationComplete",
               GATE_ARRAY_CANCELLED: "Cancelled", GATE_ARRAY_DEADLINE: "Deadline", GATE_ARRAY_NO_NEXT: "", GATE_ARRAY_TASK_LIMIT: "ArrayTaskLimit"}
GATE_AP_HAS_META, GATE_AP_HAS_PARENT, GATE_AP_COMPLETE, GATE_AP_CANCEL, GATE_AP_HAS_NEXT, GATE_AP_ALL = 1, 2, 4, 8, 16, 31


class CnsGateJobs(C.Structure):
    _fields_ = [("num_jobs", C.c_uint64), ("job_id", _P), ("held", _P), ("begin_sec", _P), ("dep_is_or", _P), ("dep_ready_sec", _P),
                ("dep_offsets", _P), ("dep_job", _P), ("dep_delay_sec", _P), ("array_parent", _P), ("ap_flags", _P), ("ap_deadline_sec", _P),
                ("ap_running", _P), ("ap_run_limit", _P)]


class CnsGateEvents(C.Structure):
    _fields_ = [("num_events", C.c_uint64), ("dependent_job_id", _P), ("dependee_job_id", _P), ("event_sec", _P)]


class CnsGateOut(C.Structure):
    _fields_ = [("code", _P), ("pending", _P), ("num_pending", _P), ("ready_sec", _P), ("dep_erased", _P), ("counts", _P), ("ev_stats", _P)]


@dataclass
class GateJobs:
    """cns_gate_jobs: the pending map in ascending job id.  None for an optional array is the header's NULL."""
    job_id: np.ndarray
    held: Optional[np.ndarray] = None
    begin_sec: Optional[np.ndarray] = None
    dep_is_or: Optional[np.ndarray] = None
    dep_ready_sec: Optional[np.ndarray] = None
    dep_offsets: Optional[np.ndarray] = None
    dep_job: Optional[np.ndarray] = None
    dep_delay_sec: Optional[np.ndarray] = None
    array_parent: Optional[np.ndarray] = None
    ap_flags: Optional[np.ndarray] = None
    ap_deadline_sec: Optional[np.ndarray] = None
    ap_running: Optional[np.ndarray] = None
    ap_run_limit: Optional[np.ndarray] = None

    _DTYPES = (("job_id", np.uint32), ("held", np.uint8), ("begin_sec", np.int64), ("dep_is_or", np.uint8), ("dep_ready_sec", np.int64),
               ("dep_offsets", np.uint64), ("dep_job", np.uint32), ("dep_delay_sec", np.uint64), ("array_parent", np.uint8), ("ap_flags", np.uint8),
               ("ap_deadline_sec", np.int64), ("ap_running", np.uint64), ("ap_run_limit", np.uint64))

    def __post_init__(self):
        for f, dt in self._DTYPES:
            a = getattr(self, f)
            if a is not None:
                setattr(self, f, _arr(a, dt))

    @property
    def num_jobs(self) -> int:
        return len(self.job_id)

    @property
    def num_entries(self) -> int:
        return 0 if self.dep_offsets is None or len(self.dep_offsets) == 0 else int(self.dep_offsets[-1])

    def to_c(self) -> CnsGateJobs:
        s = CnsGateJobs()
        s.num_jobs = self.num_jobs
        for f, _ in self._DTYPES:
            a = getattr(self, f)
            setattr(s, f, None if a is None else _ptr(a if len(a) else np.zeros(1, a.dtype)))
        return s


@dataclass
class GateEvents:
    """cns_gate_events: the dependency events in queue order."""
    dependent_job_id: np.ndarray
    dependee_job_id: np.ndarray
    event_sec: np.ndarray

    def __post_init__(self):
        self.dependent_job_id = _arr(self.dependent_job_id, np.uint32)
        n = len(self.dependent_job_id)
        self.dependee_job_id = _arr(self.dependee_job_id, np.uint32, n)
        self.event_sec = _arr(self.event_sec, np.int64, n)

    def to_c(self) -> CnsGateEvents:
        s = CnsGateEvents()
        s.num_events = len(self.dependent_job_id)
        for f in ("dependent_job_id", "dependee_job_id", "event_sec"):
            a = getattr(self, f)
            setattr(s, f, _ptr(a if len(a) else np.zeros(1, a.dtype)))
        return s


# ---- the submit limits over a batch of submissions (include/crane_gpu_submit/submit_limits.h) ----------------------------
SUBMIT_JOB_MAX_TIME_LIMIT_SEC = 315576000000   # kJobMaxTimeLimitSec
SUBMIT_CARRY = 1
SUBMIT_MAX_JOBS = 1 << 24
(SUBMIT_OK, SUBMIT_NOT_CANDIDATE, SUBMIT_BAD_COUNT, SUBMIT_BAD_REQUEST, SUBMIT_MAX_JOB_COUNT_PER_USER, SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT,
 SUBMIT_QOS_JOB_COUNT_EXCEEDED, SUBMIT_CPUS_PER_TASK_BEYOND, SUBMIT_TRES_PER_JOB_BEYOND, SUBMIT_TIME_LIMIT_BEYOND, SUBMIT_USER_ACCOUNT_MISMATCH,
 SUBMIT_PARTITION_TRES_PER_JOB_BEYOND, SUBMIT_PARTITION_TIME_BEYOND, SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER,
 SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT, SUBMIT_MAX_TRES_PER_USER_BEYOND, SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND) = range(17)
SUBMIT_STR = {SUBMIT_OK: "OK", SUBMIT_NOT_CANDIDATE: "NOT_CANDIDATE", SUBMIT_BAD_COUNT: "BAD_COUNT", SUBMIT_BAD_REQUEST: "BAD_REQUEST",
              SUBMIT_MAX_JOB_COUNT_PER_USER: "MAX_JOB_COUNT_PER_USER", SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT: "MAX_JOB_COUNT_PER_ACCOUNT",
              SUBMIT_QOS_JOB_COUNT_EXCEEDED: "QOS_JOB_COUNT_EXCEEDED", SUBMIT_CPUS_PER_TASK_BEYOND: "CPUS_PER_TASK_BEYOND",
              SUBMIT_TRES_PER_JOB_BEYOND: "TRES_PER_JOB_BEYOND", SUBMIT_TIME_LIMIT_BEYOND: "TIME_LIMIT_BEYOND",
              SUBMIT_USER_ACCOUNT_MISMATCH: "USER_ACCOUNT_MISMATCH", SUBMIT_PARTITION_TRES_PER_JOB_BEYOND: "PARTITION_TRES_PER_JOB_BEYOND",
              SUBMIT_PARTITION_TIME_BEYOND: "PARTITION_TIME_BEYOND",
              SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_USER: "PARTITION_MAX_SUBMIT_JOBS_PER_USER",
              SUBMIT_PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT: "PARTITION_MAX_SUBMIT_JOBS_PER_ACCOUNT",
              SUBMIT_MAX_TRES_PER_USER_BEYOND: "MAX_TRES_PER_USER_BEYOND", SUBMIT_MAX_TRES_PER_ACCOUNT_BEYOND: "MAX_TRES_PER_ACCOUNT_BEYOND"}
# the reference's CraneErrCode names (ERR_TIME_TIMIT_BEYOND is its spelling); "" for the three codes it has no name for
SUBMIT_ERR_NAME = {c: ("SUCCESS" if c == SUBMIT_OK else "" if c < SUBMIT_MAX_JOB_COUNT_PER_USER else
                       "ERR_TIME_TIMIT_BEYOND" if c == SUBMIT_TIME_LIMIT_BEYOND else "ERR_" + SUBMIT_STR[c]) for c in range(17)}


class CnsSubmitTables(C.Structure):
    _fields_ = [("num_users", C.c_uint32), ("num_user_accts", C.c_uint32), ("num_accounts", C.c_uint32), ("num_qos", C.c_uint32),
                ("num_partitions", C.c_uint32), ("num_part_limits", C.c_uint32), ("gres", CnsGresLayout), ("qos", _P), ("acct_parent", _P),
                ("part_limits", _P), ("user_part_limit", _P), ("acct_part_limit", _P), ("user_qos", _P), ("user_part", _P), ("acct_qos", _P),
                ("acct_part", _P), ("qos_usage", _P), ("user_qos_submit", _P), ("user_part_submit", _P), ("acct_qos_submit", _P),
                ("acct_part_submit", _P), ("qos_submit", _P), ("user_exists", _P), ("acct_exists", _P), ("qos_exists", _P)]


class CnsSubmitKeys(C.Structure):
    _fields_ = [("user", _P), ("user_acct", _P), ("account", _P), ("qos", _P), ("count", _P), ("skip", _P)]


class CnsSubmitOut(C.Structure):
    _fields_ = [("code", _P), ("time_limit_out", _P), ("num_admitted", _P)]


class CnsSubmitTiming(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("prep_ms", C.c_double), ("admit_ms", C.c_double), ("d2h_ms", C.c_double),
                ("candidates", C.c_uint64), ("admitted", C.c_uint64), ("rounds", C.c_uint32), ("ordered_fallback", C.c_uint32)]


# ---- releases and charges on the usage tables (include/crane_gpu_usage/usage.h) -------------------------------------------
USAGE_RELEASE, USAGE_CHARGE = 0, 1
USAGE_CARRY = 1
USAGE_MAX_JOBS = 1 << 24
USAGE_BIT_USER_QOS, USAGE_BIT_USER_PART, USAGE_BIT_QOS = 0, 1, 14
USAGE_SLOTS = 15          # records one row touches at the most = bits of a mask


def usage_bit_acct_qos(i):
    return 2 + 2 * i


def usage_bit_acct_part(i):
    return 3 + 2 * i


class CnsUsageTables(C.Structure):
    _fields_ = [("num_users", C.c_uint32), ("num_user_accts", C.c_uint32), ("num_accounts", C.c_uint32), ("num_qos", C.c_uint32),
                ("num_partitions", C.c_uint32), ("reserved0", C.c_uint32), ("gres", CnsGresLayout), ("acct_parent", _P),
                ("user_qos", _P), ("user_part", _P), ("acct_qos", _P), ("acct_part", _P), ("qos_usage", _P),
                ("user_qos_submit", _P), ("user_part_submit", _P), ("acct_qos_submit", _P), ("acct_part_submit", _P), ("qos_submit", _P),
                ("user_qos_exists", _P), ("user_part_exists", _P), ("acct_qos_exists", _P), ("acct_part_exists", _P),
                ("user_exists", _P), ("acct_exists", _P), ("qos_exists", _P)]


class CnsUsageJobs(C.Structure):
    _fields_ = [("num_jobs", C.c_uint64), ("user", _P), ("user_acct", _P), ("account", _P), ("qos", _P), ("partition", _P), ("cpu_raw", _P),
                ("mem", _P), ("wall_sec", _P), ("jobs_count", _P), ("submit_count", _P), ("name_total", _P), ("class_count", _P), ("skip", _P)]


class CnsUsageOut(C.Structure):
    _fields_ = [("not_found", _P), ("over_free", _P), ("num_clean", _P)]


class CnsUsageTablesOut(C.Structure):
    _fields_ = [(f, _P) for f in ("user_qos", "user_part", "acct_qos", "acct_part", "qos_usage", "user_qos_submit", "user_part_submit",
                                  "acct_qos_submit", "acct_part_submit", "qos_submit", "user_qos_exists", "user_part_exists",
                                  "acct_qos_exists", "acct_part_exists", "user_exists", "acct_exists", "qos_exists")]


class CnsUsageTiming(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("kernels_ms", C.c_double), ("d2h_ms", C.c_double), ("items", C.c_uint64), ("records", C.c_uint64)]


# ---- the running set kept on the device between two cycles (include/crane_gpu_running/running.h) ----------------------------
class CnsRunningStep(C.Structure):
    _fields_ = [("num_retire", C.c_uint64), ("retire_ids", _P), ("num_jobs", C.c_uint64), ("now_sec", C.c_int64), ("job_id", _P),
                ("admit", _P), ("reservation", _P)]


class CnsRunningStepOut(C.Structure):
    _fields_ = [("found", _P), ("num_retired", _P), ("num_admitted", _P)]


class CnsRunningLedger(C.Structure):
    _fields_ = [("capacity_jobs", C.c_uint64), ("capacity_allocs", C.c_uint64), ("num_jobs", _P), ("num_allocs", _P)] + \
               [(f, _P) for f in ("job_id", "end_sec", "reservation", "alloc_offsets", "alloc_node", "alloc_cpu_raw", "alloc_mem",
                                  "alloc_core_lo", "alloc_core_hi", "alloc_core_w2", "alloc_core_w3", "alloc_gres")]


class CnsRunningTiming(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("kernels_ms", C.c_double), ("d2h_ms", C.c_double), ("jobs", C.c_uint64), ("allocs", C.c_uint64),
                ("pairs", C.c_uint64)]


# include/crane_gpu_amend/running_amend.h
class CnsRunningAmend(C.Structure):
    _fields_ = [("num_amend", C.c_uint64), ("job_ids", _P), ("end_sec", _P)]


class CnsRunningAmendOut(C.Structure):
    _fields_ = [("found", _P), ("num_amended", _P)]


class CnsRunningAmendTiming(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("kernels_ms", C.c_double), ("d2h_ms", C.c_double), ("rows", C.c_uint64), ("pairs", C.c_uint64)]


# include/crane_gpu_running/running_preempt.h
class CnsPreemptIndexOut(C.Structure):
    _fields_ = [("capacity_entries", C.c_uint64), ("capacity_rows", C.c_uint64), ("num_entries", _P), ("num_rows", _P)] + \
               [(f, _P) for f in ("ent_job", "ent_slot", "ent_end", "rj_off", "rj_ent", "rj_end", "rj_preempting")]


class CnsRunningPreemptTiming(C.Structure):
    _fields_ = [("setup_ms", C.c_double), ("index_ms", C.c_double), ("mark_ms", C.c_double), ("entries", C.c_uint64), ("rows", C.c_uint64),
                ("index_built", C.c_uint32), ("reserved0", C.c_uint32)]


# include/crane_gpu_running/running_attrs.h
class CnsRunningAttrs(C.Structure):
    _fields_ = [(f, _P) for f in ("start_sec", "qos", "qos_priority", "partition_priority", "account")]


class CnsRunningAttrsOut(C.Structure):
    _fields_ = [("capacity_jobs", C.c_uint64), ("num_jobs", _P)] + \
               [(f, _P) for f in ("start_sec", "qos", "qos_priority", "partition_priority", "account", "node_num", "alloc_cpu_raw", "alloc_mem")]


@dataclass
class RunningAttrs:
    """cns_running_attrs: the per-job attributes beside the device ledger, one value per row (a seed) or per queue job (an advance,
    where start_sec is not read and may be left out)."""
    qos: np.ndarray
    qos_priority: np.ndarray
    partition_priority: np.ndarray
    account: np.ndarray
    start_sec: np.ndarray = None

    def __post_init__(self):
        self.qos = _arr(self.qos, np.uint32); n = len(self.qos)
        self.qos_priority = _arr(self.qos_priority, np.uint32, n)
        self.partition_priority = _arr(self.partition_priority, np.uint32, n)
        self.account = _arr(self.account, np.uint32, n)
        if self.start_sec is not None:
            self.start_sec = _arr(self.start_sec, np.int64, n)

    def __len__(self):
        return len(self.qos)

    def to_c(self) -> CnsRunningAttrs:
        return CnsRunningAttrs(*[_ptr(getattr(self, f)) for f, _ in CnsRunningAttrs._fields_])


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64) if len(lists) else []
    flat = np.asarray([int(v) for x in lists for v in x], np.uint32)
    return off, flat


@dataclass
class CommitEvents:
    """cns_commit_events: what LockAndGetResReduceEvents() holds, split by alternative.
    node_events: [(time_sec, [node, ...]), ...];  affected_resv: [(resv index, exists, end_sec, [node, ...]), ...]."""
    node_events: list = field(default_factory=list)
    affected_resv: list = field(default_factory=list)

    def __post_init__(self):
        self.ev_time_sec = np.asarray([int(t) for t, _ in self.node_events], np.int64)
        self.ev_offsets, self.ev_nodes = _csr([n for _, n in self.node_events])
        self.ar_resv = np.asarray([int(a[0]) for a in self.affected_resv], np.uint32)
        self.ar_exists = np.asarray([1 if a[1] else 0 for a in self.affected_resv], np.uint8)
        self.ar_end_sec = np.asarray([int(a[2]) for a in self.affected_resv], np.int64)
        self.ar_offsets, self.ar_nodes = _csr([a[3] for a in self.affected_resv])

    def to_c(self) -> CnsCommitEvents:
        s = CnsCommitEvents()
        s.num_node_events, s.num_affected_resv = len(self.ev_time_sec), len(self.ar_resv)
        for f, _ in CnsCommitEvents._fields_[2:]:
            a = getattr(self, f)
            setattr(s, f, _ptr(a if len(a) else np.zeros(1, a.dtype)))
        return s


@dataclass
class CommitJobs:
    """cns_commit_jobs: the queue of the last cycle.  time_limit_sec / reservation as given to the cycle, gone[j] != 0: no longer in the
    pending map; preempt_offsets / preempted: the cycle's PreemptOut; running_alive[r] != 0: running job r is still in the running map."""
    time_limit_sec: np.ndarray
    reservation: Optional[np.ndarray] = None
    gone: Optional[np.ndarray] = None
    preempt_offsets: Optional[np.ndarray] = None
    preempted: Optional[np.ndarray] = None
    running_alive: Optional[np.ndarray] = None

    def __post_init__(self):
        self.time_limit_sec = _arr(self.time_limit_sec, np.int64)
        n = len(self.time_limit_sec)
        if self.reservation is not None:
            self.reservation = _arr(self.reservation, np.uint32, n)
        if self.gone is not None:
            self.gone = _arr(self.gone, np.uint8, n)
        if self.preempt_offsets is not None:
            self.preempt_offsets = _arr(self.preempt_offsets, np.uint64, n + 1)
            self.preempted = _arr(self.preempted if self.preempted is not None else [], np.uint32)
        if self.running_alive is not None:
            self.running_alive = _arr(self.running_alive, np.uint8)

    @property
    def num_jobs(self) -> int:
        return len(self.time_limit_sec)

    def to_c(self) -> CnsCommitJobs:
        s = CnsCommitJobs()
        s.num_jobs = self.num_jobs
        for f in ("time_limit_sec", "reservation", "gone", "preempt_offsets", "preempted", "running_alive"):
            a = getattr(self, f)
            setattr(s, f, None if a is None else _ptr(a if len(a) else np.zeros(1, a.dtype)))
        s.num_running = 0 if self.running_alive is None else len(self.running_alive)
        return s
