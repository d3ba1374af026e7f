"""A condition on the inputs of tests/test_gpu_running_amend.py, checked on the oracle alone: in every scenario the amendment changes
the next cycle — the oracle's start times or fp64 node costs differ between the old and the amended running set.  Without it a call
that skipped the refill of the per-slot tables would pass the GPU test.  No GPU, no engine."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import running_amend_case as ac
from tests import running_amend_pyref as ap
from tests.test_gpu_running import NOW


def _cycle(cluster, led, jobs, resv=None, now=NOW):
    run, ids = led.arrays()
    return pyoracle.select(cluster, jobs, now, running=run if len(ids) else None, reservations=resv)


def differs(a, b, J):
    return (not np.array_equal(a.placements.start_sec[:J], b.placements.start_sec[:J]) or not np.array_equal(a.placements.reason[:J], b.placements.reason[:J])
            or not np.array_equal(a.costs().view(np.uint64), b.costs().view(np.uint64)))


@pytest.mark.parametrize("name,build", ac.all_cases(), ids=[n for n, _ in ac.all_cases()])
def test_the_amendment_changes_the_next_cycle(built, name, build):
    c = build()
    before = _cycle(c.cluster, c.led, c.jobs, c.resv)
    led = c.led.copy()
    found, n = ap.amend(led, c.ids, c.ends)
    assert n >= 1 and n == int(found.sum())
    after = _cycle(c.cluster, led, c.jobs, c.resv)
    J = c.jobs.num_jobs
    assert differs(before, after, J), f"{name}: the oracle's cycle is the same with and without the amendment"
    # the pinned jobs wait for the amended rows: a start moved to one of the new ends
    assert set(after.placements.start_sec[:J].tolist()) & set(c.ends), name


def test_the_hand_case_starts_where_the_running_job_ends(built):
    cluster, led, jobs = ac.hand_case()
    starts = []
    for end in (NOW + 1000, NOW + 500, NOW + 2000):
        ap.amend(led, [1], [end])
        pl = _cycle(cluster, led, jobs).placements
        assert int(pl.reason[0]) == 2, "it waits for resources, with a start planned"
        starts.append(int(pl.start_sec[0]))
    assert starts == [NOW + 1000, NOW + 500, NOW + 2000]


def test_the_stale_tables_scenario(built):
    c, flipped = ac.stale_case()
    led = c.led.copy()
    ap.amend(led, c.ids, c.ends)
    assert differs(_cycle(flipped, c.led, c.jobs), _cycle(flipped, led, c.jobs), c.jobs.num_jobs)


def test_the_composition_scenario(built):
    """Amend, advance with retire and admit, amend an admitted row: both amendments change the cycle behind them."""
    p = ac.composition_plan()
    led = p.led.copy()
    first = _cycle(p.cluster, led, p.jobs, now=p.now)
    amended = led.copy()
    ap.amend(amended, p.ids, p.ends)
    cyc = _cycle(p.cluster, amended, p.jobs, now=p.now)
    assert differs(first, cyc, p.jobs.num_jobs)
    amended.retire(p.retire)
    assert amended.admit(cyc.placements, p.jobs.time_limit_sec, p.now, p.job_ids) >= 3
    ids2, ends2 = p.second(amended)
    again = amended.copy()
    found, n = ap.amend(again, ids2, ends2)
    assert n == len(ids2) and all(i >= 50000 for i in ids2), "admitted rows"
    assert differs(_cycle(p.cluster, amended, p.jobs2, now=p.now + 60), _cycle(p.cluster, again, p.jobs2, now=p.now + 60), p.jobs2.num_jobs)


def test_the_reservation_what_if_scenario(built):
    """On tests/resvq_pyref.py: the amended end moves a candidate from RUNNING to FREE at the given start, and the other way round, and
    moves an earliest start."""
    from tests import resvq_pyref as rq
    w = ac.what_if_case()
    s0 = rq.NodeState(w.cluster.num_nodes, w.led.arrays()[0], w.resv)
    a0 = rq.answer(s0, NOW, w.queries)
    led = w.led.copy()
    ap.amend(led, w.ids, w.ends)
    a1 = rq.answer(rq.NodeState(w.cluster.num_nodes, led.arrays()[0], w.resv), NOW, w.queries)
    c0, c1 = a0["code"].tolist(), a1["code"].tolist()
    assert any(x == rq.RUNNING and y == rq.FREE for x, y in zip(c0, c1)) and any(x == rq.FREE and y == rq.RUNNING for x, y in zip(c0, c1))
    e = np.nonzero(w.queries.find_earliest)[0]
    assert len(e) and (a0["status"][e] == rq.OK).all() and (a1["status"][e] == rq.OK).all() and (a0["start_sec"][e] != a1["start_sec"][e]).all()
