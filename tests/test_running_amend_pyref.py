"""tests/running_amend_pyref.py, the truth the amended device ledger is held to, against a small table worked out by hand.  No GPU, no
engine."""
import numpy as np
import pytest

from cranesched_amd import abi
from tests import running_amend_pyref as ap
from tests import running_pyref as rp


def _seed():
    """Three running jobs: A (id 7) on nodes 0 and 4, B (id 3) without an allocation, C (id 9) on node 2 inside reservation 1."""
    run = abi.Running(end_sec=[1100, 1200, 1300], alloc_offsets=[0, 2, 2, 3], alloc_node=[0, 4, 2], alloc_cpu_raw=[256, 512, 768],
                      alloc_mem=[1, 2, 3], alloc_core_lo=[1, 3, 7], alloc_core_hi=[0, 0, 8], alloc_gres=[0, 0, 0xF0],
                      reservation=[abi.RESV_NONE, abi.RESV_NONE, 1])
    return rp.Ledger.from_running(run, [7, 3, 9])


def _rest(led):
    """Everything of the ledger but its ends."""
    run, ids = led.arrays()
    return [list(ids)] + [list(getattr(run, f)) for f in rp.RUN_FIELDS if f != "end_sec"]


def _ends(led):
    return [r.end_sec for r in led.rows]


def test_one_row_and_nothing_else_moves():
    led = _seed()
    rest = _rest(led)
    found, n = ap.amend(led, [3], [5000])
    assert list(found) == [1] and n == 1
    assert _ends(led) == [1100, 5000, 1300] and _rest(led) == rest


def test_an_unknown_id_changes_nothing():
    led = _seed()
    before = led.copy()
    found, n = ap.amend(led, [8], [5000])
    assert list(found) == [0] and n == 0
    assert rp.same_ledger(led.arrays(), before.arrays()) is None


def test_unknown_ids_among_known_ones_in_the_callers_order():
    led = _seed()
    found, n = ap.amend(led, [9, 8, 7, 0], [1, 2, 3, 4])
    assert list(found) == [1, 0, 1, 0] and n == 2
    assert _ends(led) == [3, 1200, 1]


def test_all_rows():
    led = _seed()
    rest = _rest(led)
    found, n = ap.amend(led, [9, 3, 7], [-1, rp.I64_MAX, rp.I64_MIN])
    assert list(found) == [1, 1, 1] and n == 3
    assert _ends(led) == [rp.I64_MIN, rp.I64_MAX, -1] and _rest(led) == rest


def test_none():
    led = _seed()
    before = led.copy()
    found, n = ap.amend(led, [], [])
    assert len(found) == 0 and n == 0 and found.dtype == np.uint8
    assert rp.same_ledger(led.arrays(), before.arrays()) is None


def test_the_same_end_as_before_counts_as_written():
    led = _seed()
    before = led.copy()
    found, n = ap.amend(led, [7, 9], [1100, 1300])
    assert list(found) == [1, 1] and n == 2
    assert rp.same_ledger(led.arrays(), before.arrays()) is None


def test_an_empty_ledger():
    led = rp.Ledger()
    found, n = ap.amend(led, [1, 2], [10, 20])
    assert list(found) == [0, 0] and n == 0 and led.rows == []


def test_an_id_twice_is_the_callers_mistake():
    with pytest.raises(AssertionError):
        ap.amend(_seed(), [7, 7], [1, 2])
