"""tests/running_pyref.py, the truth of the device ledger, against a small table worked out by hand.  No GPU, no engine."""
import numpy as np

from cranesched_amd import abi
from tests import running_pyref as rp

NOW = 1000


def _seed():
    """Three running jobs: A (id 7) on nodes 0 and 4, B (id 3) without an allocation, C (id 9) on node 2 inside reservation 1."""
    run = abi.Running(end_sec=[1100, 1200, 1300], alloc_offsets=[0, 2, 2, 3], alloc_node=[0, 4, 2], alloc_cpu_raw=[256, 512, 768],
                      alloc_mem=[1, 2, 3], alloc_core_lo=[1, 3, 7], alloc_core_hi=[0, 0, 8], alloc_gres=[0, 0, 0xF0],
                      reservation=[abi.RESV_NONE, abi.RESV_NONE, 1])
    return rp.Ledger.from_running(run, [7, 3, 9])


def _queue():
    """Five queue jobs: 0 starts now on node 1; 1 is backfilled (start later); 2 failed (reason Resource); 3 starts now on two records of
    which the second names no node; 4 starts now on nodes 3 and 5, inside reservation 0."""
    pl = abi.Placements(5, 6)
    pl.start_sec[:] = [NOW, NOW + 60, 0, NOW, NOW]
    pl.reason[:] = [0, 0, 2, 0, 0]
    pl.place_offsets[:] = [0, 1, 2, 2, 4, 6]
    pl.node_idx[:] = [1, 2, 0, abi.NODE_NONE, 3, 5]
    pl.cpu_raw[:] = [10, 20, 30, 0, 40, 50]
    pl.mem[:] = [11, 21, 31, 0, 41, 51]
    pl.core_lo[:] = [12, 22, 32, 0, 42, 52]
    pl.core_hi[:] = [13, 23, 33, 0, 43, 53]
    pl.core_w2[:] = [14, 24, 34, 0, 44, 54]
    pl.core_w3[:] = [15, 25, 35, 0, 45, 55]
    pl.gres[:] = [16, 26, 36, 0, 46, 56]
    limit = np.array([100, 100, 100, (1 << 63) - 1, 7], np.int64)
    resv = np.array([abi.RESV_NONE] * 4 + [0], np.uint32)
    return pl, limit, resv


def _table(led):
    run, ids = led.arrays()
    return (list(ids), list(run.end_sec), list(run.reservation), list(run.alloc_offsets), list(run.alloc_node), list(run.alloc_cpu_raw),
            list(run.alloc_gres))


def test_seed_keeps_the_input_order():
    assert _table(_seed()) == ([7, 3, 9], [1100, 1200, 1300], [abi.RESV_NONE, abi.RESV_NONE, 1], [0, 2, 2, 3], [0, 4, 2], [256, 512, 768], [0, 0, 0xF0])


def test_retire_first_last_unknown_all():
    led = _seed()
    found, n = led.retire([7])                       # the first row
    assert list(found) == [1] and n == 1 and led.ids() == [3, 9]
    assert _table(led)[3:5] == ([0, 0, 1], [2])
    led = _seed()
    found, n = led.retire([9])                       # the last row
    assert list(found) == [1] and n == 1 and _table(led)[0:5] == ([7, 3], [1100, 1200], [abi.RESV_NONE] * 2, [0, 2, 2], [0, 4])
    led = _seed()
    found, n = led.retire([12, 3])                   # an unknown id changes nothing (CranedMetaContainer.cpp:248-253)
    assert list(found) == [0, 1] and n == 1 and led.ids() == [7, 9]
    assert _table(led)[3:5] == ([0, 2, 3], [0, 4, 2])
    led = _seed()
    found, n = led.retire([9, 7, 3])                 # any order; all
    assert list(found) == [1, 1, 1] and n == 3 and _table(led) == ([], [], [], [0], [], [], [])


def test_admit_with_a_mask():
    led = _seed()
    pl, limit, resv = _queue()
    n = led.admit(pl, limit, NOW, [20, 21, 22, 23, 24], admit=[1, 1, 1, 0, 1], reservation=resv)
    assert n == 2                                    # 1 did not start now, 2 failed, 3 is masked out
    ids, end, rv, off, node, cpu, gres = _table(led)
    assert ids == [7, 3, 9, 20, 24] and end == [1100, 1200, 1300, NOW + 100, NOW + 7]
    assert rv == [abi.RESV_NONE, abi.RESV_NONE, 1, abi.RESV_NONE, 0]        # a job inside a reservation keeps it
    assert off == [0, 2, 2, 3, 4, 6] and node == [0, 4, 2, 1, 3, 5] and cpu == [256, 512, 768, 10, 40, 50] and gres == [0, 0, 0xF0, 16, 46, 56]
    run, _ = led.arrays()
    assert list(run.alloc_mem[3:]) == [11, 41, 51] and list(run.alloc_core_lo[3:]) == [12, 42, 52] and list(run.alloc_core_hi[3:]) == [13, 43, 53]
    assert list(run.alloc_core_w2[3:]) == [14, 44, 54] and list(run.alloc_core_w3[3:]) == [15, 45, 55]


def test_admit_without_a_mask_a_record_without_a_node_and_a_saturating_end():
    led = _seed()
    pl, limit, _ = _queue()
    n = led.admit(pl, limit, NOW, [20, 21, 22, 23, 24])
    assert n == 3
    ids, end, rv, off, node, cpu, _ = _table(led)
    assert ids == [7, 3, 9, 20, 23, 24]
    assert end[4] == (1 << 63) - 1                                           # start + limit saturates, as absl::Time does
    assert off == [0, 2, 2, 3, 4, 5, 7] and node == [0, 4, 2, 1, 0, 3, 5]    # job 23: the CNS_NODE_NONE record is no allocation
    assert rv[3:] == [abi.RESV_NONE] * 3 and cpu[3:] == [10, 30, 40, 50]


def test_a_job_that_did_not_start_never_enters():
    led = rp.Ledger()
    pl, limit, _ = _queue()
    pl.start_sec[:] = NOW + 1
    assert led.admit(pl, limit, NOW, [20, 21, 22, 23, 24]) == 0 and led.rows == []
    pl.start_sec[:] = NOW
    pl.reason[:] = 1
    assert led.admit(pl, limit, NOW, [20, 21, 22, 23, 24]) == 0 and led.rows == []


def test_same_ledger_names_the_field():
    a, b = _seed(), _seed()
    assert rp.same_ledger(a.arrays(), b.arrays()) is None
    b.rows[2].end_sec += 1
    assert rp.same_ledger(a.arrays(), b.arrays()) == "end_sec"
    b = _seed()
    b.rows[0], b.rows[1] = b.rows[1], b.rows[0]
    assert rp.same_ledger(a.arrays(), b.arrays()) == "job_id"
