"""The running ledger of include/crane_gpu_running/running.h in plain Python: a list of rows in ledger order.  Seeding keeps the input
order, a retire deletes by id (a stable erase), an admit appends the started jobs of a cycle in queue order.  This is the truth the
device ledger is held to; what a cycle makes of it comes from the existing yardsticks (cns_set_running and the oracle) fed with
arrays() — never from the code under test."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from cranesched_amd import abi

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
PLANES = ("cpu_raw", "mem", "core_lo", "core_hi", "core_w2", "core_w3", "gres")


@dataclass
class Row:
    job_id: int
    end_sec: int
    reservation: int = abi.RESV_NONE
    allocs: list = field(default_factory=list)   # [(node, {plane: value})]


class Ledger:
    def __init__(self, rows=None):
        self.rows = list(rows or [])

    @classmethod
    def from_running(cls, running: "abi.Running | None", job_ids) -> "Ledger":
        rows = []
        if running is not None:
            for j in range(len(running.end_sec)):
                resv = int(running.reservation[j]) if running.reservation is not None else abi.RESV_NONE
                al = []
                for a in range(int(running.alloc_offsets[j]), int(running.alloc_offsets[j + 1])):
                    al.append((int(running.alloc_node[a]), {
                        "cpu_raw": int(running.alloc_cpu_raw[a]), "mem": int(running.alloc_mem[a]), "core_lo": int(running.alloc_core_lo[a]),
                        "core_hi": int(running.alloc_core_hi[a]), "gres": int(running.alloc_gres[a]),
                        "core_w2": int(running.alloc_core_w2[a]) if running.alloc_core_w2 is not None else 0,
                        "core_w3": int(running.alloc_core_w3[a]) if running.alloc_core_w3 is not None else 0}))
                rows.append(Row(int(job_ids[j]), int(running.end_sec[j]), resv, al))
        return cls(rows)

    def copy(self) -> "Ledger":
        return Ledger([Row(r.job_id, r.end_sec, r.reservation, list(r.allocs)) for r in self.rows])

    def ids(self):
        return [r.job_id for r in self.rows]

    def retire(self, ids):
        """-> (found per id, rows erased).  An id no row carries changes nothing (CranedMetaContainer.cpp:248-253)."""
        ids = [int(i) for i in ids]
        assert len(set(ids)) == len(ids), "retire ids are distinct"
        have = set(self.ids())
        found = [1 if i in have else 0 for i in ids]
        gone = set(ids)
        before = len(self.rows)
        self.rows = [r for r in self.rows if r.job_id not in gone]
        return np.array(found, np.uint8), before - len(self.rows)

    def admit(self, placements: abi.Placements, time_limit_sec, now: int, job_ids, admit=None, reservation=None) -> int:
        """Appends, in queue order, every job with admit[j] set (None: all) whose reason is REASON_NONE and whose start is `now`:
        end = start + time_limit (saturating), its reservation, one allocation per placement record that names a node."""
        n = 0
        for j in range(placements.num_jobs):
            if admit is not None and not admit[j]:
                continue
            if int(placements.reason[j]) != 0 or int(placements.start_sec[j]) != now:
                continue
            end = min(max(int(placements.start_sec[j]) + int(time_limit_sec[j]), I64_MIN), I64_MAX)
            al = []
            for x in range(int(placements.place_offsets[j]), int(placements.place_offsets[j + 1])):
                if int(placements.node_idx[x]) == abi.NODE_NONE:
                    continue
                al.append((int(placements.node_idx[x]), {p: int(getattr(placements, p)[x]) for p in PLANES}))
            self.rows.append(Row(int(job_ids[j]), end, int(reservation[j]) if reservation is not None else abi.RESV_NONE, al))
            n += 1
        return n

    def arrays(self):
        """-> (abi.Running with every plane, job ids): what cns_running_get returns, and what cns_set_running takes."""
        off = np.zeros(len(self.rows) + 1, np.uint32)
        off[1:] = np.cumsum([len(r.allocs) for r in self.rows], dtype=np.uint64) if self.rows else []
        flat = [a for r in self.rows for a in r.allocs]
        u64 = lambda p: np.array([a[1][p] for a in flat], np.uint64)
        run = abi.Running(end_sec=np.array([r.end_sec for r in self.rows], np.int64), alloc_offsets=off,
                          alloc_node=np.array([a[0] for a in flat], np.uint32), alloc_cpu_raw=np.array([a[1]["cpu_raw"] for a in flat], np.int64),
                          alloc_mem=u64("mem"), alloc_core_lo=u64("core_lo"), alloc_core_hi=u64("core_hi"), alloc_gres=u64("gres"),
                          reservation=np.array([r.reservation for r in self.rows], np.uint32), alloc_core_w2=u64("core_w2"), alloc_core_w3=u64("core_w3"))
        return run, np.array(self.ids(), np.uint32)


RUN_FIELDS = ("end_sec", "alloc_offsets", "alloc_node", "alloc_cpu_raw", "alloc_mem", "alloc_core_lo", "alloc_core_hi", "alloc_gres",
              "reservation", "alloc_core_w2", "alloc_core_w3")


def same_ledger(got, want):
    """None, or the first field in which two (abi.Running, ids) pairs differ."""
    (gr, gi), (wr, wi) = got, want
    if not np.array_equal(np.asarray(gi, np.uint32), np.asarray(wi, np.uint32)):
        return "job_id"
    for f in RUN_FIELDS:
        a, b = getattr(gr, f), getattr(wr, f)
        if a.shape != b.shape or not np.array_equal(a, b):
            return f
    return None
