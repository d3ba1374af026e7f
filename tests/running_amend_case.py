"""The scenarios of tests/test_gpu_running_amend.py, built without a GPU so that tests/test_running_amend_effect.py can hold each of
them to a condition on the oracle alone: the amendment changes the next cycle.  A scenario is a cluster, a ledger (tests/running_pyref.py),
the amendments (ids and new ends, in the caller's order) and the queue of the cycle that follows.  The small inputs are those of
tests/test_gpu_running.py; every queue ends with one job per amended row that is pinned to that row's first node and asks for all of
its cores, so that the job starts when the node's last allocation ends."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from cranesched_amd import abi
from tests import running_pyref as rp
from tests.test_gpu_running import FULL, GIB, NOW, _resv, _shared_cluster, flat_cluster, running

U32_MAX = 0xFFFFFFFF
SIZES = ["0", "1", "63", "64", "65", "chunk-1", "chunk", "chunk+1", "scan carry"]
ENTRIES = [255, 256, 257]
KS = ["K=1", "K=2", "K=R", "K=R+3"]
LAYOUTS = ["shared partitions", "reservations"]


def shape():
    """cns_running_shape: (job_chunk, lane_max_allocs, sort_tile, scan_span).  Needs no GPU."""
    from cranesched_amd.engine import lib
    v = [C.c_uint32(0) for _ in range(4)]
    assert lib().cns_running_shape(*[C.byref(x) for x in v]) == 0
    return [x.value for x in v]


@dataclass
class Case:
    name: str
    cluster: "abi.Cluster"
    led: "rp.Ledger"
    ids: list            # the amendments, in the caller's order
    ends: list
    jobs: "abi.Jobs"
    resv: "abi.Reservations | None" = None
    entries: "int | None" = None   # (slot, allocation) pairs of the ledger's tables, where the scenario is about them


def mixed_queue(widths, pinned, partition=None, cpus=128, resv=None):
    """One job per entry of widths (that many nodes, one task of one cpu each), then one job per node of `pinned`: one node, `cpus`
    cores, and only that node allowed."""
    k = np.array(list(widths) + [1] * len(pinned), np.uint32)
    j = len(k)
    cpu = np.array([256] * len(widths) + [cpus * 256] * len(pinned), np.int64)
    off, flat = [0], []
    for _ in widths:
        off.append(len(flat))
    for n in pinned:
        flat.append(int(n))
        off.append(len(flat))
    part = np.zeros(j, np.uint32) if partition is None else np.asarray(list(partition) + [0] * (j - len(partition)), np.uint32)
    return abi.Jobs(partition=part, time_limit_sec=600 + 60 * np.arange(j, dtype=np.int64), node_mem=np.zeros(j, np.uint64), task_cpu_raw=cpu,
                    task_mem=np.full(j, GIB, np.uint64), node_num=k, ntasks=k, ntasks_per_node_min=np.ones(j, np.uint32), ntasks_per_node_max=np.ones(j, np.uint32),
                    reservation=resv, incl_offsets=np.array(off, np.uint64), incl_nodes=np.array(flat or [0], np.uint32))


def _first_nodes(led, ids):
    by_id = {r.job_id: r for r in led.rows}
    return [by_id[i].allocs[0][0] for i in ids if i in by_id and by_id[i].allocs]


def _later(k, base=5000):
    """k new ends far behind every end the ledgers below are built with, all different."""
    return [NOW + base + 37 * i for i in range(k)]


def size_case(which) -> Case:
    """R one-allocation rows on 300 nodes (more than 256 slots); the first, a middle and the last row amended, and an id no row carries."""
    job_chunk, _, _, scan_span = shape()
    R = {"chunk-1": job_chunk - 1, "chunk": job_chunk, "chunk+1": job_chunk + 1, "scan carry": 64 * scan_span + 1}.get(which)
    R = int(which) if R is None else R
    n = 300
    led = running(n, [1] * R)
    rows = led.ids()
    hit = sorted({rows[0], rows[len(rows) // 2], rows[-1]}, reverse=True) if rows else []
    ids = hit[:1] + [77] + hit[1:]
    return Case(f"{which} rows", flat_cluster(n), led, ids, _later(len(ids)), mixed_queue([1, 2, 1, 3], _first_nodes(led, hit)))


def entries_case(m) -> Case:
    """m table entries: the refill's workgroup holds 256."""
    n = 300
    led = running(n, [1] * m)
    rows = led.ids()
    ids = [rows[-1], rows[m // 2], rows[0]]
    return Case(f"{m} entries", flat_cluster(n), led, ids, _later(3), mixed_queue([1, 2], _first_nodes(led, ids)), entries=m)


def k_case(which) -> Case:
    """A ledger of six rows.  The ids 0 and 2^32 - 1 stand at the ends of the bisection: as rows of the ledger (hits) for K = 1, 2, R,
    and as ids no row carries (misses) for K = R + 3.  The amendments come in descending order."""
    n = 12
    led = running(n, [1, 2, 1, 3, 1, 2], stride=5)
    R = len(led.rows)
    if which != "K=R+3":
        for r, i in zip(led.rows, [9, 0, 4000, U32_MAX, 17, 5]):
            r.job_id = i
    have = sorted(led.ids(), reverse=True)
    ids = {"K=1": [0], "K=2": [U32_MAX, 0], "K=R": have, "K=R+3": sorted(have + [U32_MAX, 77, 0], reverse=True)}[which]
    assert len(ids) == {"K=1": 1, "K=2": 2, "K=R": R, "K=R+3": R + 3}[which] and ids == sorted(ids, reverse=True)
    return Case(which, flat_cluster(n), led, ids, _later(len(ids)), mixed_queue([1, 2], _first_nodes(led, ids)))


def widths_case() -> Case:
    """Rows of 1, lane_max_allocs, lane_max_allocs + 1, 64 and 65 allocations, each amended: csr_owner over wide rows."""
    lane_max = shape()[1]
    widths = [1, lane_max, lane_max + 1, 64, 65]
    n = 160
    led = running(n, [2] + widths + widths[::-1] + [3], stride=11)
    ids = led.ids()[1:6][::-1]
    assert [len(r.allocs) for r in led.rows[1:6]] == widths
    return Case("row widths", flat_cluster(n), led, ids, _later(5), mixed_queue([1, 2, 1], _first_nodes(led, ids)))


def layout_case(which) -> Case:
    if which == "shared partitions":
        # three partitions over the same nodes (an allocation is 1, 2 or 3 table entries); node 5 is not schedulable (no entry at all)
        n = 40
        led = running(n, [1, 2, 3, 1, 9, 1, 1, 2] * 6, stride=3)
        on5 = [r.job_id for r in led.rows if any(a[0] == 5 for a in r.allocs)]
        assert on5
        ids = sorted(set(led.ids()[::5]) | set(on5), reverse=True)
        pinned = [x for x in _first_nodes(led, ids) if x != 5]
        entries = sum(1 + (a[0] % 2 == 0) + (a[0] % 3 == 0) for r in led.rows for a in r.allocs if a[0] != 5)
        assert entries > sum(len(r.allocs) for r in led.rows)
        return Case(which, _shared_cluster(n), led, ids, _later(len(ids)), mixed_queue([1, 2, 1, 3, 1, 1], pinned, partition=[0, 1, 2, 0, 1, 2]), entries=entries)
    # an active reservation over nodes 2, 3, 4 (the low 64 cores of each): rows 901, 902 run inside it (a virtual slot), 903 names a
    # reservation the snapshot does not know, 905 runs inside it on a node it does not list; every row is amended
    n = 24
    rv = _resv([2, 3, 4], NOW - 100, NOW + 50000)
    rows = []
    for i, (node, r) in enumerate(zip([2, 2, 3, 6, 3, 7], [abi.RESV_NONE, 0, 0, 5, abi.RESV_NONE, 0])):
        rows.append(rp.Row(900 + i, NOW + 500 + i, r, [(node, {"cpu_raw": 256, "mem": GIB, "core_lo": (1 << i) if r == 0 else 0, "core_hi": 0 if r == 0 else (1 << i),
                                                               "core_w2": 0, "core_w3": 0, "gres": 0})]))
    led = rp.Ledger(rows)
    ids = led.ids()[::-1]
    jobs = mixed_queue([1, 1, 2, 1], [2, 3], partition=[0, 1, 0, 0], cpus=64, resv=np.array([abi.RESV_NONE, 0, 0, abi.RESV_NONE, abi.RESV_NONE, abi.RESV_NONE], np.uint32))
    return Case(which, flat_cluster(n, [np.arange(n), np.arange(0, n, 2)]), led, ids, _later(6), jobs, resv=rv, entries=2 + 1 + 1 + 0 + 1 + 0)


def hand_case():
    """One node, one running job (id 1) that holds all 128 cores until NOW + 1000, one queue job that asks for all of them."""
    al = [(0, {"cpu_raw": 128 * 256, "mem": GIB, "core_lo": int(FULL), "core_hi": int(FULL), "core_w2": 0, "core_w3": 0, "gres": 0})]
    led = rp.Ledger([rp.Row(1, NOW + 1000, abi.RESV_NONE, al)])
    return flat_cluster(1), led, mixed_queue([], [0])


def all_cases():
    """(name, builder) of every scenario whose amendment must change the next cycle."""
    out = [(f"{w} rows", lambda w=w: size_case(w)) for w in SIZES if w != "0"]
    out += [(f"{m} entries", lambda m=m: entries_case(m)) for m in ENTRIES]
    out += [(w, lambda w=w: k_case(w)) for w in KS]
    out += [("row widths", widths_case)]
    out += [(w, lambda w=w: layout_case(w)) for w in LAYOUTS]
    return out


def stale_case():
    """-> (Case, the cluster with one node flipped to not schedulable): cns_set_nodes between the seed and the amend empties the
    per-slot tables, the amend writes the ledger alone, the advance behind it rebuilds."""
    c = size_case("65")
    sched = np.ones(c.cluster.num_nodes, np.uint8)
    flip = next(r.allocs[0][0] for r in c.led.rows if r.job_id not in c.ids)
    assert flip not in _first_nodes(c.led, c.ids)
    sched[flip] = 0
    return c, flat_cluster(c.cluster.num_nodes, sched=sched)


@dataclass
class Plan:
    cluster: "abi.Cluster"
    led: "rp.Ledger"
    jobs: "abi.Jobs"
    jobs2: "abi.Jobs"
    now: int
    ids: list
    ends: list
    retire: list
    job_ids: np.ndarray

    def second(self, led):
        """The second amendment: the first and the last admitted row of `led` (ids from 50000) end much later."""
        adm = [i for i in led.ids() if i >= 50000]
        return [adm[-1], adm[0]], [self.now + 60 + 9000, self.now + 60 + 9100]


def composition_plan() -> Plan:
    """A busy small cluster (the case of tests/test_gpu_running.py's retire / admit test): amend two seeded rows, a cycle, a boundary that
    retires two rows and admits the started jobs, amend two admitted rows, the same queue again."""
    from tests import helpers
    cluster, jobs, now, run = helpers.random_case(21, N=24, J=120, P=2, running=20)
    led = rp.Ledger.from_running(run, 1000 + np.arange(len(run.end_sec)))
    ids = led.ids()
    return Plan(cluster, led, jobs, jobs, now, [ids[-1], ids[len(ids) // 2]], [now + 7000, now + 7100], [ids[1], ids[3]], 50000 + np.arange(jobs.num_jobs))


@dataclass
class WhatIf:
    cluster: "abi.Cluster"
    led: "rp.Ledger"
    resv: "abi.Reservations"
    ids: list
    ends: list
    queries: "abi.ResvQueries"


def what_if_case() -> WhatIf:
    """Eight nodes.  Row 1 on node 0 ends at NOW + 100, row 2 on node 1 at NOW + 1000, row 3 on nodes 1 and 3 at NOW + 50; node 2 is
    reserved over [NOW + 400, NOW + 700).  Query 0 asks at NOW + 500 for one of nodes 0, 1, 2, 9: free, running, reserved, not found.
    Query 1 asks for the earliest start of both nodes 0 and 1: NOW + 1000.  The amendment swaps the two ends' roles: row 1 to NOW + 800,
    row 2 to NOW + 200 — node 0 becomes running and node 1 free at NOW + 500, the earliest start moves to NOW + 800."""
    one = {"cpu_raw": 256, "mem": GIB, "core_lo": 1, "core_hi": 0, "core_w2": 0, "core_w3": 0, "gres": 0}
    two = dict(one, core_lo=2)
    led = rp.Ledger([rp.Row(1, NOW + 100, abi.RESV_NONE, [(0, dict(one))]), rp.Row(2, NOW + 1000, abi.RESV_NONE, [(1, dict(one))]),
                     rp.Row(3, NOW + 50, abi.RESV_NONE, [(1, dict(two)), (3, dict(one))])])
    q = abi.ResvQueries([NOW + 500, NOW], [100, 100], [1, 2], [0, 4, 6], [0, 1, 2, 9, 0, 1], [0, 1])
    return WhatIf(flat_cluster(8), led, _resv([2], NOW + 400, NOW + 700), [2, 1], [NOW + 200, NOW + 800], q)
