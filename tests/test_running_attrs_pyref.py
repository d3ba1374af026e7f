"""tests/running_attrs_pyref.py against hand cases: the columns follow the rows through seed, retire and admit, the per-row sums are
exact, and the order of the rows decides the last bit of an account's fp64 service value (the case tests/test_gpu_prio_resident.py
relies on).  No GPU, no native code."""
import struct

import numpy as np

from cranesched_amd import abi
from tests import prio_pyref
from tests import running_attrs_pyref as rap
from tests import running_pyref as rp

NOW = 1_700_000_000


def _alloc(node, cpu, mem):
    return (node, {"cpu_raw": cpu, "mem": mem, "core_lo": 0, "core_hi": 0, "core_w2": 0, "core_w3": 0, "gres": 0})


def _ledger():
    rows = [rp.Row(10, NOW + 5, abi.RESV_NONE, [_alloc(0, 256, 100)]),
            rp.Row(11, NOW + 6, abi.RESV_NONE, [_alloc(1, 512, 7), _alloc(2, 256, 9)]),
            rp.Row(12, NOW + 7, abi.RESV_NONE, []),
            rp.Row(13, NOW + 8, abi.RESV_NONE, [_alloc(3, 1, 1)])]
    attrs = {"start_sec": [NOW - 10, NOW - 20, NOW - 30, NOW - 40], "qos": [0, 1, 2, 3], "qos_priority": [5, 6, 7, 8], "partition_priority": [1, 2, 3, 4],
             "account": [2, 0, 2, 1]}
    return rap.AttrLedger(rp.Ledger(rows), attrs)


def test_seed_keeps_the_input_order_and_sums_the_allocations():
    led = _ledger()
    c, d = led.columns(), led.derived()
    assert list(c["account"]) == [2, 0, 2, 1] and c["start_sec"].dtype == np.int64 and c["qos"].dtype == np.uint32
    assert list(d["node_num"]) == [1, 2, 0, 1] and list(d["alloc_cpu_raw"]) == [256, 768, 0, 1] and list(d["alloc_mem"]) == [100, 16, 0, 1]


def test_a_retire_erases_the_attributes_with_the_row_stably():
    led = _ledger()
    found, n = led.retire([12, 99, 10])
    assert list(found) == [1, 0, 1] and n == 2
    assert led.ledger.ids() == [11, 13] and list(led.columns()["qos_priority"]) == [6, 8] and list(led.columns()["start_sec"]) == [NOW - 20, NOW - 40]


def test_an_admitted_row_takes_the_queue_jobs_attributes_and_starts_now():
    led = _ledger()
    pl = abi.Placements(3, 3)
    pl.reason[:3] = [0, 3, 0]
    pl.start_sec[:3] = [NOW, 0, NOW]
    pl.place_offsets[:4] = [0, 1, 2, 3]
    pl.node_idx[:3] = [4, abi.NODE_NONE, 5]
    pl.cpu_raw[:3] = [256, 0, 512]
    pl.mem[:3] = [11, 0, 22]
    qa = {"qos": [3, 2, 1], "qos_priority": [30, 20, 10], "partition_priority": [9, 8, 7], "account": [1, 1, 0], "start_sec": [1, 2, 3]}
    n = led.admit(pl, np.array([60, 60, 60]), NOW, [50, 51, 52], qa, admit=np.array([1, 1, 1], np.uint8))
    assert n == 2 and led.ledger.ids() == [10, 11, 12, 13, 50, 52]
    c = led.columns()
    assert list(c["start_sec"][-2:]) == [NOW, NOW], "start_sec of the queue is not read"
    assert list(c["qos"][-2:]) == [3, 1] and list(c["account"][-2:]) == [1, 0] and list(led.derived()["alloc_mem"][-2:]) == [11, 22]
    other = led.copy()
    other.retire([50])
    assert len(led.rows) == 6 and len(other.rows) == 5


def test_sums_outside_their_type_and_the_least_bad_row():
    big = 1 << 62
    rows = [rp.Row(1, NOW, abi.RESV_NONE, [_alloc(0, 5, 5)]),
            rp.Row(2, NOW, abi.RESV_NONE, [_alloc(0, big, 1), _alloc(1, big, 1)]),               # 2^63: outside int64
            rp.Row(3, NOW, abi.RESV_NONE, [_alloc(0, 1, (1 << 64) - 1), _alloc(1, 1, 1)]),       # 2^64: outside uint64
            rp.Row(4, NOW, abi.RESV_NONE, [_alloc(0, -3, 1), _alloc(1, 1, 1)])]
    attrs = {"start_sec": [NOW] * 4, "qos": [0] * 4, "qos_priority": [0] * 4, "partition_priority": [0] * 4, "account": [0, 1, 1, 7]}
    led = rap.AttrLedger(rp.Ledger(rows), attrs)
    assert led.first_bad_row(8) == (1, "range")
    assert led.derived()["alloc_cpu_raw"][1] == -(1 << 63) and led.derived()["alloc_mem"][2] == 0
    led.retire([2])
    assert led.first_bad_row(8) == (1, "range")
    led.retire([3])
    assert led.first_bad_row(8) == (1, "negative") and led.first_bad_row(7) == (1, "account") and led.first_bad_row(1) == (1, "account")
    led.retire([4])
    assert led.first_bad_row(1) is None


def spread_rows(n=24):
    """Account 1: rows whose service terms span more than twenty binades (start times about 2^k seconds back).  Summed front to back and
    back to front the fp64 results differ — the small terms are absorbed one way and accumulate the other.  Account 0: two long-running
    rows, the largest service value; account 2 has no row (the least).  So the fair-share factor of a pending job of account 1 is
    1 - acc[1] / acc[0] and carries the difference."""
    rows = [rp.Row(100 + i, NOW + 100, abi.RESV_NONE, [_alloc(i % 4, 256 * (1 + i % 3), 1000 + 37 * i)]) for i in range(n + 2)]
    attrs = {"start_sec": [NOW - (3 << i) - i for i in range(n)] + [NOW - (1 << 27), NOW - (1 << 26)], "qos": [0] * (n + 2), "qos_priority": [10] * (n + 2),
             "partition_priority": [1] * (n + 2), "account": [1] * n + [0, 0]}
    return rap.AttrLedger(rp.Ledger(rows), attrs)


PENDING = [dict(submit=NOW - 100, qos=10, part=1, nodes=1, cpu_raw=256, mem=1000, account=0),
           dict(submit=NOW - 5000, qos=100, part=5, nodes=2, cpu_raw=1024, mem=5000, account=1),
           dict(submit=NOW - 900, qos=10, part=1, nodes=1, cpu_raw=512, mem=2000, account=2)]
CFG = dict(max_age=14 * 86400, w_age=0, w_fair=1, w_size=0, w_part=0, w_qos=0, favor_small=True)   # the priority IS the fair-share factor


def test_the_order_of_the_rows_decides_the_last_bits():
    led = spread_rows()
    fwd = prio_pyref.bounds(NOW, CFG["max_age"], PENDING, led.pyref_running())["acc"]
    back = prio_pyref.bounds(NOW, CFG["max_age"], PENDING, led.pyref_running()[::-1])["acc"]
    assert fwd[1] != back[1] and abs(fwd[1] - back[1]) <= 1e-9 * fwd[1], "the same terms in another order: another fp64 sum"
    assert struct.pack("<d", fwd[1]) != struct.pack("<d", back[1])
    assert fwd[0] > fwd[1] > fwd[2] == 0.0
    a = prio_pyref.ordered(NOW, CFG, PENDING, led.pyref_running())[1]
    b = prio_pyref.ordered(NOW, CFG, PENDING, led.pyref_running()[::-1])[1]
    assert a[1] != b[1] and 0.0 < a[1] < 1.0, "... and it shows in the priority of the job of account 1"
