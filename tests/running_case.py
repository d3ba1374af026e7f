"""Several consecutive scheduling cycles, each built from the previous one's results: the scenario the device ledger of
include/crane_gpu_running/running.h is held to.  One tests/helpers.random_case cluster (96 nodes, 2 partitions, GRES), about 40 running
jobs, a fresh queue of 300 pending jobs per cycle, `now` advancing by STEP seconds.  Behind every cycle: retire every ledger job whose
end is not after the next cycle's now, admit every second job the cycle started (the mask stands in for the run limits).  Everything
here comes from the oracle and tests/running_pyref.py; tests/test_running_case.py checks it without a GPU, tests/test_gpu_running.py
replays it on the device."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from cranesched_amd import abi
from oracle import pyoracle
from tests import helpers
from tests import running_pyref as rp

STEP = 600
CYCLES = 4
N, P, J, RUNNING = 96, 2, 300, 40


@dataclass
class Cycle:
    now: int
    jobs: abi.Jobs
    before: rp.Ledger          # the ledger the cycle runs on
    oracle: object             # pyoracle.OracleRun of the cycle on before.arrays()
    retire: np.ndarray         # the boundary behind the cycle: ids to retire,
    job_ids: np.ndarray        # ... the ids of the queue's jobs,
    admit: np.ndarray          # ... the mask,
    found: np.ndarray          # ... and what it answers
    num_retired: int
    num_admitted: int
    after: rp.Ledger


def scenario(seed: int, cycles: int = CYCLES, case=None):
    """-> (cluster, first ledger, [Cycle]).  case: a generator with tests.helpers.random_case's signature (default: that one), e.g.
    tests.gres_wide.wide_case_of(layout): its queues must fit the cluster of every seed."""
    case = case or helpers.random_case
    cluster, jobs0, now0, run0 = case(seed, N=N, J=J, P=P, running=RUNNING)
    led = rp.Ledger.from_running(run0, 1000 + np.arange(len(run0.end_sec)))
    first = led.copy()
    out = []
    for c in range(cycles):
        now = now0 + STEP * c
        jobs = jobs0 if c == 0 else case(seed * 16 + c, N=N, J=J, P=P, running=0)[1]
        before = led.copy()
        run, _ = before.arrays()
        ora = pyoracle.select(cluster, jobs, now, running=run)
        pl = ora.placements
        started = np.nonzero((pl.reason[:J] == 0) & (pl.start_sec[:J] == now))[0]
        admit = np.zeros(J, np.uint8)
        admit[started[::2]] = 1
        job_ids = (10000 * (c + 1) + np.arange(J)).astype(np.uint32)
        retire = np.array([r.job_id for r in led.rows if r.end_sec <= now + STEP], np.uint32)
        found, nret = led.retire(retire)
        nadm = led.admit(pl, jobs.time_limit_sec, now, job_ids, admit)
        out.append(Cycle(now, jobs, before, ora, retire, job_ids, admit, found, nret, nadm, led.copy()))
    return cluster, first, out


def touched_nodes(cluster: abi.Cluster, *ledgers, placements=None):
    """The nodes a running allocation or a placement names."""
    s = set()
    for led in ledgers:
        for r in led.rows:
            s.update(n for n, _ in r.allocs)
    if placements is not None:
        used = placements.node_idx[:placements.capacity]
        s.update(int(n) for n in used[used != abi.NODE_NONE])
    return sorted(n for n in s if n < cluster.num_nodes)
