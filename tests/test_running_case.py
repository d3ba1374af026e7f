"""tests/running_case.py, the multi-cycle scenario of the device ledger, on the oracle alone: every cycle admits and retires enough that
the GPU test (tests/test_gpu_running.py) cannot pass vacuously, ids stay distinct, the ledgers chain.  No GPU."""
import numpy as np
import pytest

from tests import running_case as rc
from tests import running_pyref as rp

SEEDS = (11, 12)


@pytest.fixture(scope="module", params=SEEDS)
def scen(built, request):
    return rc.scenario(request.param)


def test_every_cycle_admits_and_retires(scen):
    cluster, first, cycles = scen
    assert len(cycles) == rc.CYCLES == 4 and cluster.num_nodes == 96 and cluster.num_partitions == 2 and cluster.gres_slots.any()
    assert 30 <= len(first.rows) <= 40
    for c in cycles:
        assert c.jobs.num_jobs == 300
        assert c.num_admitted >= 10, "a condition on the inputs: the cycle feeds the next one"
        assert c.num_retired >= 1 and c.found.all() and len(c.retire) == c.num_retired
        started = (c.oracle.placements.reason[:300] == 0) & (c.oracle.placements.start_sec[:300] == c.now)
        assert c.num_admitted == int((started & (c.admit != 0)).sum()) < int(started.sum()), "the mask holds some started jobs back"
        # backfilled and failed jobs are in every queue, and none of them enters
        pl = c.oracle.placements
        assert ((pl.reason[:300] != 0) & (pl.start_sec[:300] > c.now)).any(), "a job with a start time in the future (backfilled behind others)"
        assert ((pl.reason[:300] != 0) & (pl.start_sec[:300] == 0)).any(), "a job without a start time"
        entered = set(c.after.ids()) - set(c.before.ids())
        assert entered == set(int(i) for i in c.job_ids[started & (c.admit != 0)])


def test_the_ledgers_chain_and_ids_stay_distinct(scen):
    _, first, cycles = scen
    prev = first
    for c in cycles:
        assert rp.same_ledger(c.before.arrays(), prev.arrays()) is None
        ids = c.after.ids()
        assert len(set(ids)) == len(ids)
        assert all(r.end_sec > c.now + rc.STEP for r in c.after.rows if r.job_id in set(c.before.ids())), "what ended by the next now is gone"
        # a stable erase, then an append: the survivors keep their order in front
        keep = [i for i in c.before.ids() if i not in set(int(x) for x in c.retire)]
        assert ids[:len(keep)] == keep
        prev = c.after


def test_multi_node_jobs_enter_with_all_their_records(scen):
    _, _, cycles = scen
    widest = max(len(r.allocs) for c in cycles for r in c.after.rows)
    assert widest >= 2
    run, _ = cycles[-1].after.arrays()
    assert int(run.alloc_offsets[-1]) == len(run.alloc_node) > len(run.end_sec) - 5
    assert np.all(np.diff(run.alloc_offsets.astype(np.int64)) >= 0)
