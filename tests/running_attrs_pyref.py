"""The attribute columns of include/crane_gpu_running/running_attrs.h in plain Python, built on tests/running_pyref.py: one dict of
attributes per ledger row, carried through seed, retire (a stable erase) and admit (appended in queue order, start = now), and the
three values the sorter derives per row from the row's allocations (exact Python integers: a sum that leaves its type is seen as
such).  This is the truth running_attrs() of the device is held to; what the sorter makes of it comes from cns_priority_order and
tests/prio_pyref.py fed with these rows — never from the code under test."""
from __future__ import annotations

import numpy as np

from cranesched_amd import abi
from cranesched_amd.priority import PrioRunning
from tests import running_pyref as rp

COLUMNS = ("start_sec", "qos", "qos_priority", "partition_priority", "account")
QUEUE_COLUMNS = COLUMNS[1:]
DERIVED = ("node_num", "alloc_cpu_raw", "alloc_mem")
I64_MAX, I64_MIN, U64_MAX = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1


def random_attrs(rng, n: int, accounts: int, now: int, start: bool = True) -> dict:
    """Seeded attributes for n rows (or n queue jobs: start=False)."""
    a = {"qos": rng.integers(0, 4, n), "qos_priority": rng.choice([0, 10, 100, 1000], n), "partition_priority": rng.choice([1, 5, 50], n),
         "account": rng.integers(0, max(accounts, 1), n)}
    if start:
        a["start_sec"] = now - rng.integers(1, 5 * 86400, n)
    return {k: [int(x) for x in v] for k, v in a.items()}


def to_abi(attrs: dict) -> abi.RunningAttrs:
    return abi.RunningAttrs(qos=attrs["qos"], qos_priority=attrs["qos_priority"], partition_priority=attrs["partition_priority"], account=attrs["account"],
                            start_sec=attrs.get("start_sec"))


class AttrLedger:
    """A tests/running_pyref.Ledger and, row for row, its attributes."""

    def __init__(self, ledger: rp.Ledger, attrs: dict):
        self.ledger = ledger
        self.rows = [{c: int(attrs[c][i]) for c in COLUMNS} for i in range(len(ledger.rows))]
        assert all(len(attrs[c]) == len(ledger.rows) for c in COLUMNS)

    def copy(self) -> "AttrLedger":
        return AttrLedger(self.ledger.copy(), self.columns())

    def retire(self, ids):
        gone = {int(i) for i in ids}
        self.rows = [a for a, r in zip(self.rows, self.ledger.rows) if r.job_id not in gone]
        return self.ledger.retire(ids)

    def admit(self, placements, time_limit_sec, now: int, job_ids, queue_attrs: dict, admit=None, reservation=None) -> int:
        before = len(self.ledger.rows)
        n = self.ledger.admit(placements, time_limit_sec, now, job_ids, admit, reservation)
        taken = [j for j in range(placements.num_jobs)
                 if (admit is None or admit[j]) and int(placements.reason[j]) == 0 and int(placements.start_sec[j]) == now]
        assert len(taken) == n and [self.ledger.rows[before + k].job_id for k in range(n)] == [int(job_ids[j]) for j in taken]
        for j in taken:
            row = {c: int(queue_attrs[c][j]) for c in QUEUE_COLUMNS}
            row["start_sec"] = int(now)
            self.rows.append(row)
        return n

    def columns(self) -> dict:
        dt = {"start_sec": np.int64}
        return {c: np.array([a[c] for a in self.rows], dt.get(c, np.uint32)) for c in COLUMNS}

    def sums(self):
        """Per row (node_num, cpu, mem) as exact integers."""
        return [(len(r.allocs), sum(a[1]["cpu_raw"] for a in r.allocs), sum(a[1]["mem"] for a in r.allocs)) for r in self.ledger.rows]

    def derived(self) -> dict:
        """What running_attrs() reports: the low 64 bits of the sums."""
        s = self.sums()
        cpu = np.array([((c + (1 << 63)) & U64_MAX) - (1 << 63) for _, c, _ in s], np.int64)
        return {"node_num": np.array([n for n, _, _ in s], np.uint32), "alloc_cpu_raw": cpu, "alloc_mem": np.array([m & U64_MAX for _, _, m in s], np.uint64)}

    def first_bad_row(self, num_accounts: int):
        """None, or (row, kind) of the least row cns_priority_order_resident refuses: 'account', 'range' (a sum outside its type) or
        'negative' (cpu), in that order on one row."""
        for i, ((_, c, m), a) in enumerate(zip(self.sums(), self.rows)):
            if a["account"] >= num_accounts:
                return i, "account"
            if c > I64_MAX or c < I64_MIN or m > U64_MAX:
                return i, "range"
            if c < 0:
                return i, "negative"
        return None

    def prio_running(self) -> PrioRunning:
        """The rows as the host-fed sorter takes them, ledger order."""
        c, d = self.columns(), self.derived()
        return PrioRunning(start_sec=c["start_sec"], qos_priority=c["qos_priority"], partition_priority=c["partition_priority"], node_num=d["node_num"],
                           alloc_cpu_raw=d["alloc_cpu_raw"], alloc_mem=d["alloc_mem"], account=c["account"])

    def pyref_running(self):
        """... and as tests/prio_pyref.py takes them."""
        return [dict(start=a["start_sec"], qos=a["qos_priority"], part=a["partition_priority"], nodes=n, cpu_raw=c, mem=m, account=a["account"])
                for a, (n, c, m) in zip(self.rows, self.sums())]


def same_attrs(got: dict, want: AttrLedger):
    """None, or the first field in which running_attrs() differs from the reference."""
    exp = {**want.columns(), **want.derived()}
    for f in COLUMNS + DERIVED:
        if got[f].shape != exp[f].shape or got[f].dtype != exp[f].dtype or not np.array_equal(got[f], exp[f]):
            return f
    return None
