"""tests/running_preempt_pyref.py against a table derived by hand.  Four nodes; node 2 is not schedulable.  Partition 0 lists nodes
0, 1, 2 and partition 1 nodes 1, 3: they share node 1, so they form one group whose slots are partition 0's schedulable nodes, then
partition 1's:  slot 0 = node 0, slot 1 = node 1 (in partition 0), slot 2 = node 1 (in partition 1), slot 3 = node 3.  Reservation 0
covers node 3: its virtual slot is 4.

The ledger, in ledger order:
  row 0  id 100, ends 1050, inside reservation 0, one allocation on node 3          -> one entry, on slot 4
  row 1  id 101, ends 1300, one allocation on node 2 (not schedulable)               -> no entry
  row 2  id 102, ends 1500, two allocations on node 1 (which sits in two partitions) -> two entries on slot 1, two on slot 2
Entries by slot, inside a slot in ledger order:  d = 0, 1 on slot 1 (row 2), d = 2, 3 on slot 2 (row 2), d = 4 on slot 4 (row 0).
Rows -> entries: row 0 -> [4], row 1 -> [], row 2 -> [0, 1, 2, 3].
The preempting set is {102, 999} at now = 1000: 102 runs (row 2), 999 does not and is dropped.  Row 2's entries end at 1001; row 0's
keep 1050.  rj_end = max(end, now + 1) for a row with an entry: 1050, 0 (no entry), 1001."""
import numpy as np

from cranesched_amd import abi
from tests import running_preempt_pyref as rpp
from tests import running_pyref as rp

GIB = 1 << 30
FULL = np.uint64(0xFFFFFFFFFFFFFFFF)


def _alloc(node, core):
    return (node, {"cpu_raw": 256, "mem": GIB, "core_lo": 1 << core, "core_hi": 0, "core_w2": 0, "core_w3": 0, "gres": 0})


def _ledger():
    return rp.Ledger([rp.Row(100, 1050, 0, [_alloc(3, 0)]), rp.Row(101, 1300, abi.RESV_NONE, [_alloc(2, 0)]),
                      rp.Row(102, 1500, abi.RESV_NONE, [_alloc(1, 0), _alloc(1, 1)])])


NODE_SLOTS = [[0], [1, 2], [], [3]]
RESV_SLOTS = [(4, [3])]


def test_the_layout_of_the_hand_derived_cluster():
    n = 4
    cluster = abi.Cluster(np.full(n, 64 * 256, np.int64), np.full(n, 64 * GIB, np.uint64), np.full(n, FULL), np.zeros(n, np.uint64), np.zeros(n, np.uint64),
                          np.array([0, 3, 5], np.uint32), np.array([0, 1, 2, 1, 3], np.uint32), schedulable=np.array([1, 1, 0, 1], np.uint8))
    resv = abi.Reservations(start_sec=[900], end_sec=[5000], alloc_offsets=[0, 1], alloc_node=[3], alloc_cpu_raw=[8 * 256], alloc_mem=[8 * GIB],
                            alloc_core_lo=[0xFF], alloc_core_hi=[0], alloc_gres=[0])
    assert rpp.layout_of(cluster, resv) == (NODE_SLOTS, RESV_SLOTS)
    assert rpp.layout_of(cluster) == (NODE_SLOTS, [])


def test_entry_order_is_by_slot_then_by_ledger_row():
    assert rpp.entry_order(_ledger(), NODE_SLOTS, RESV_SLOTS) == [(1, 2), (1, 2), (2, 2), (2, 2), (4, 0)]
    # an unknown reservation, and one that does not list the node: no entry
    led = rp.Ledger([rp.Row(1, 10, 7, [_alloc(3, 0)]), rp.Row(2, 10, 0, [_alloc(0, 0)])])
    assert rpp.entry_order(led, NODE_SLOTS, RESV_SLOTS) == []


def test_index_of_the_hand_derived_table():
    x = rpp.index(_ledger(), NODE_SLOTS, RESV_SLOTS, 1000, [102, 999])
    assert x["ent_slot"].tolist() == [1, 1, 2, 2, 4]
    assert x["ent_job"].tolist() == [2, 2, 2, 2, 0]
    assert x["rj_off"].tolist() == [0, 1, 1, 5]
    assert x["rj_ent"].tolist() == [4, 0, 1, 2, 3]
    assert x["rj_preempting"].tolist() == [0, 0, 1]
    assert x["ent_end"].tolist() == [1001, 1001, 1001, 1001, 1050]
    assert x["rj_end"].tolist() == [1050, 0, 1001]
    assert x["set_in"] == [102]


def test_a_row_that_ended_long_ago_ends_at_now_plus_one_for_the_trees_only():
    """now = 2000: no row is marked, the per-slot ends are the ledger's, rj_end is lifted to now + 1 (JobScheduler.cpp:6513-6514)."""
    x = rpp.index(_ledger(), NODE_SLOTS, RESV_SLOTS, 2000, [999, 999])
    assert x["rj_preempting"].tolist() == [0, 0, 0] and x["set_in"] == []
    assert x["ent_end"].tolist() == [1500, 1500, 1500, 1500, 1050]
    assert x["rj_end"].tolist() == [2001, 0, 2001]


def test_an_empty_ledger():
    x = rpp.index(rp.Ledger([]), NODE_SLOTS, RESV_SLOTS, 1000, [5])
    assert x["rj_off"].tolist() == [0] and all(len(x[f]) == 0 for f in rpp.INDEX_FIELDS if f != "rj_off") and x["set_in"] == []
    assert rpp.same_index(x, x) is None
