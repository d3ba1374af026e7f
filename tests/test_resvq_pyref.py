"""Hand-derived cases for tests/resvq_pyref.py, the restatement of JobScheduler::CreateResv_'s node walk (JobScheduler.cpp:4383-4419)
that the GPU answers of include/crane_gpu_resv/resv_probe.h are compared with: every boundary of the two comparisons (:4395, :4405),
the node count, the earliest-start search.  The expected values are worked out by hand in the comments, not by the code under test."""
import numpy as np

from cranesched_amd import abi
from tests import resvq_pyref as ref

INF = ref.INT64_MAX


def state(num_nodes, job_ends=None, resv=None):
    s = ref.NodeState(num_nodes)
    for n, ends in (job_ends or {}).items():
        s.job_ends[n] = list(ends)
    for n, iv in (resv or {}).items():
        s.resv[n] = list(iv)
    return s


def test_running_boundary():
    """:4395 job_end > start conflicts: an end AT the start is free, one second later conflicts."""
    s = state(2, job_ends={0: [100], 1: [101]})
    ok, nf, codes, chosen = ref.at_start(s, 100, 50, 1, [0, 1])
    assert (ok, nf, codes, chosen) == (True, 1, [ref.FREE, ref.RUNNING], [0])


def test_reservation_boundaries():
    """:4405 st < end && ed > start, request [100, 150): a reservation that ends at 100 or begins at 150 is free; moved by one second
    (ends at 101, begins at 149) it conflicts."""
    s = state(4, resv={0: [(50, 100)], 1: [(150, 200)], 2: [(50, 101)], 3: [(149, 200)]})
    ok, nf, codes, chosen = ref.at_start(s, 100, 50, 2, [0, 1, 2, 3])
    assert codes == [ref.FREE, ref.FREE, ref.RESERVED, ref.RESERVED]
    assert (ok, nf, chosen) == (True, 2, [0, 1])


def test_running_is_tested_first():
    s = state(1, job_ends={0: [500]}, resv={0: [(0, 1000)]})
    assert ref.at_start(s, 100, 50, 1, [0])[2] == [ref.RUNNING]


def test_expired_reservations_and_any_running_job_count():
    """An expired reservation is an interval like any other (:4405 has no `now`); the latest of several running ends decides."""
    s = state(2, job_ends={0: [10, 300, 20]}, resv={1: [(0, 50)]})
    assert ref.at_start(s, 100, 50, 0, [0, 1])[2] == [ref.RUNNING, ref.FREE]
    assert ref.at_start(s, 40, 5, 0, [0, 1])[2] == [ref.RUNNING, ref.RESERVED]


def _queries(rows):
    """rows of (start, duration, node_num, candidates, find_earliest)"""
    off = np.concatenate([[0], np.cumsum([len(r[3]) for r in rows])])
    return abi.ResvQueries([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], off,
                           np.array([n for r in rows for n in r[3]], np.uint32), [r[4] for r in rows])


def test_node_num():
    """Nodes 0..4, node 1 busy until 500, node 3 reserved [0, 500): 3 free at 100.  node_num 0 = all five -> not enough; 1 -> the
    first free; 3 = num_free -> exactly the free ones in list order; 4 = num_free + 1 -> not enough, nothing chosen."""
    s = state(5, job_ends={1: [500]}, resv={3: [(0, 500)]})
    lst = [4, 3, 2, 1, 0]
    out = ref.answer(s, 0, _queries([(100, 50, k, lst, 0) for k in (0, 1, 3, 4)]))
    assert out["status"].tolist() == [ref.NOT_ENOUGH, ref.OK, ref.OK, ref.NOT_ENOUGH]
    assert out["num_free"].tolist() == [3, 3, 3, 3]
    assert out["start_sec"].tolist() == [0, 100, 100, 0]
    assert out["code"].tolist() == [0, 2, 0, 1, 0] * 4
    assert out["chosen_offsets"].tolist() == [0, 0, 1, 4, 4]
    assert out["chosen_nodes"].tolist() == [4, 4, 2, 0]


def test_not_found_counts_towards_all():
    """node_num 0 over [0, 7, 1] on a 2-node cluster: k = 3 although only two nodes exist (:4357-4358, :4385-4388) -> not enough;
    with node_num 2 the two found nodes do."""
    s = state(2)
    out = ref.answer(s, 0, _queries([(100, 50, 0, [0, 7, 1], 0), (100, 50, 2, [0, 7, 1], 0), (100, 50, 0, [0, 7, 1], 1)]))
    assert out["status"].tolist() == [ref.NOT_ENOUGH, ref.OK, ref.NOT_ENOUGH]
    assert out["code"].tolist() == [0, 3, 0] * 3
    assert out["chosen_nodes"].tolist() == [0, 1]


def test_earliest_count_falls_then_rises():
    """Two nodes, two wanted for 100 s from 0.  Node 0 is busy until 50.  Node 1 is free at 0 but reserved [120, 300): from start 21
    on a 100 s window runs into it.  At 0: only node 1.  At 50: node 0 is free, node 1 is blocked (50 + 100 > 120) — the count fell
    before it could reach 2.  At 300 both are free: the answer, not 50."""
    s = state(2, job_ends={0: [50]}, resv={1: [(120, 300)]})
    assert ref.rise_times(s, 0, [0, 1]) == [0, 50, 300]
    t, ok, nf, codes, chosen = ref.earliest(s, 0, 100, 2, [0, 1])
    assert (t, ok, nf, codes, chosen) == (300, True, 2, [0, 0], [0, 1])
    # one node is enough at once, and with a window of 20 s the two fit at 50: 50 + 20 <= 120
    assert ref.earliest(s, 0, 100, 1, [0, 1])[:2] == (0, True)
    assert ref.earliest(s, 0, 20, 2, [0, 1])[:2] == (50, True)


def test_earliest_overlapping_reservations():
    """Node 0 is listed by [100, 200) and [150, 400) (the table does not forbid it): the end of the first, 200, is a rise time at
    which the node is still reserved; it frees at 400."""
    s = state(1, resv={0: [(100, 200), (150, 400)]})
    assert ref.earliest(s, 90, 50, 1, [0])[:2] == (400, True)
    assert ref.earliest(s, 10, 90, 1, [0])[:2] == (10, True)      # [10, 100) ends where the first begins


def test_earliest_never():
    """A job that never ends, a reservation that never ends: the node is never free again, INT64_MAX is not a start."""
    s = state(2, job_ends={0: [INF]}, resv={1: [(500, INF)]})
    t, ok, nf, codes, chosen = ref.earliest(s, 1000, 10, 1, [0, 1])
    assert (t, ok, nf, codes, chosen) == (None, False, 0, [ref.RUNNING, ref.RESERVED], [])
    out = ref.answer(s, 0, _queries([(1000, 10, 1, [0, 1], 1), (100, 10, 1, [0, 1], 1)]))
    assert out["status"].tolist() == [ref.NOT_ENOUGH, ref.OK] and out["start_sec"].tolist() == [0, 100]   # node 1 before its reservation
    assert out["chosen_nodes"].tolist() == [1]


def test_in_the_past():
    """:4323 end_time <= now.  A start in the past alone is only a warning (:4326)."""
    s = state(1)
    out = ref.answer(s, 1000, _queries([(900, 100, 1, [0], 0), (900, 101, 1, [0], 0), (0, 5, 0, [0, 9], 1)]))
    assert out["status"].tolist() == [ref.IN_THE_PAST, ref.OK, ref.IN_THE_PAST]
    assert out["start_sec"].tolist() == [0, 900, 0] and out["num_free"].tolist() == [0, 1, 0]
    assert out["code"].tolist() == [0, 0, 0, 0] and out["chosen_nodes"].tolist() == [0]


def test_state_from_the_tables():
    """NodeState from abi.Running / abi.Reservations: every allocation of a job carries the job's end, whichever reservation it runs in."""
    z = lambda m: np.zeros(m, np.uint64)
    run = abi.Running([700, 900], [0, 2, 3], [0, 2, 2], np.zeros(3, np.int64), z(3), z(3), z(3), z(3), reservation=[abi.RESV_NONE, 0])
    rv = abi.Reservations([100], [200], [0, 2], [2, 1], np.zeros(2, np.int64), z(2), z(2), z(2), z(2))
    s = ref.NodeState(3, run, rv)
    assert s.job_ends == [[700], [], [700, 900]] and s.resv == [[], [(100, 200)], [(100, 200)]]
