"""tests/gate_pyref.py, the restatement of JobScheduler.cpp:1353-1413 that cns_gate_pending is held to, against the hand-derived table
of tests/gate_case.py: code, pending reason, ready_time and the entries left, row by row; then the properties of the whole drain that a
single row cannot show (queue order, the event statistics, the order of pending_jobs).  No GPU involved."""
import copy

import numpy as np
import pytest

from cranesched_amd import abi
from tests import gate_case as gc
from tests import gate_pyref as ref

TABLE = gc.table()


@pytest.mark.parametrize("row", TABLE, ids=[t[0] for t in TABLE])
def test_table_row(row):
    name, now, job, events, code, ready, left = row
    j = copy.deepcopy(job)
    res = ref.gate(now, [j], events)
    assert int(res.code[0]) == code, f"{abi.GATE_STR[int(res.code[0])]}, want {abi.GATE_STR[code]}"
    assert res.reasons[0] == abi.GATE_REASON[code] == ref.REASON[code]
    assert int(res.ready_sec[0]) == ready == j.dependencies.ready_time
    assert len(j.dependencies.deps) == left
    ok = code in (ref.OK, ref.OK_ARRAY_PARENT)
    assert res.pending.tolist() == ([0] if ok else []) and res.materializes == ([code == ref.OK_ARRAY_PARENT] if ok else [])
    assert int(res.counts[code]) == 1 and int(res.counts.sum()) == 1
    assert int(res.ev_stats.sum()) == len(events)


def test_the_table_names_every_case_the_header_lists():
    names = {t[0] for t in TABLE}
    assert {"and_last_arrives_met", "and_last_arrives_a_second_early", "or_one_of_three", "or_inf_entries_left", "or_last_erased_by_inf",
            "and_inf_entries_left", "and_repeat_first_wins", "or_repeat_first_wins", "delay_overflow", "delay_2_63", "event_ninf",
            "held_and_unmet"} <= names
    assert {int(t[4]) for t in TABLE} == set(range(12)), "every code of the header appears"
    assert abi.GATE_TIME_INFINITE_FUTURE == ref.INF and abi.GATE_TIME_INFINITE_PAST == ref.NINF


def test_the_repeat_rows_would_differ_had_the_second_event_applied():
    """The table's two repeat rows decide something: with the events swapped the other time is the first and the code changes."""
    for name, want_swapped in (("and_repeat_first_wins", ref.DEPENDENCY), ("or_repeat_first_wins", ref.OK)):
        _, now, job, events, code, _, _ = next(t for t in TABLE if t[0] == name)
        res = ref.gate(now, [copy.deepcopy(job)], events[::-1])
        assert int(res.code[0]) == want_swapped != code


def test_saturating_sum():
    f = ref.time_plus_seconds
    assert f(ref.INF, 0) == ref.INF and f(ref.INF, (1 << 64) - 1) == ref.INF
    assert f(ref.NINF, 0) == ref.NINF and f(ref.NINF, (1 << 64) - 1) == ref.NINF
    assert f(0, (1 << 63) - 1) == ref.INF and f(-1, (1 << 63) - 1) == ref.INF - 1 and f(-1, 1 << 63) == ref.INF
    assert f(ref.NINF + 1, (1 << 63) - 1) == 0 and f(ref.INF - 1, 0) == ref.INF - 1 and f(ref.INF - 1, 1) == ref.INF


def test_events_in_queue_order_and_their_statistics():
    jobs = [ref.Job(30, dependencies=gc.deps({1: 0, 2: 0})), ref.Job(10, dependencies=gc.deps({1: 5}, True, ref.INF)), ref.Job(20)]
    events = [(10, 1, 100), (30, 2, 700), (10, 1, 50), (40, 1, 0), (20, 1, 0), (30, 1, 900), (30, 1, 100), (5, 5, 5)]
    res = ref.gate(gc.NOW, jobs, events)
    # rows are in ascending job id whatever the order given: 10, 20, 30
    assert res.code.tolist() == [ref.OK, ref.OK, ref.OK] and res.pending.tolist() == [0, 1, 2]
    assert res.ready_sec.tolist() == [105, ref.NINF, 900]
    assert res.ev_stats.tolist() == [3, 2, 3]        # applied; jobs 40 and 5 are not pending; (10,1) again, (20,1), (30,1) again
    assert res.counts.tolist() == [3] + [0] * 15
    assert jobs[0].dependencies.deps == {} and jobs[1].dependencies.deps == {}


def test_pending_is_in_map_order_with_both_kinds():
    jobs = [ref.Job(5, held=True), ref.Job(4, array=ref.ArrayParent()), ref.Job(3, begin_time=gc.NOW + 1), ref.Job(2), ref.Job(1, array=ref.ArrayParent(cancel=True))]
    res = ref.gate(gc.NOW, jobs, [])
    assert res.code.tolist() == [ref.ARRAY_CANCELLED, ref.OK, ref.BEGIN_TIME, ref.OK_ARRAY_PARENT, ref.HELD]
    assert res.pending.tolist() == [1, 3] and res.materializes == [False, True]
    assert res.reasons == ["Cancelled", "", "BeginTime", "", "Held"]


def test_an_empty_map_ignores_every_event():
    res = ref.gate(gc.NOW, [], [(1, 2, 3), (4, 5, 6)])
    assert len(res.code) == 0 and len(res.pending) == 0 and res.ev_stats.tolist() == [0, 2, 0] and int(res.counts.sum()) == 0


def test_the_seam_cases_cover_what_they_claim():
    """The case list of the GPU test, with the shipped shape: every code, both OK kinds, wide lists in lanes 0 and 63, the first-wins rule
    deciding, events of every miss class; expected() leaves its input alone."""
    cases = gc.seam_cases(256, 8, 256)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    seen = set()
    for name, now, jobs, events in cases:
        if name.startswith("scan_") or name.startswith("random"):
            continue
        before = copy.deepcopy(jobs)
        res, erased, after = gc.expected(now, jobs, events)
        assert [j.dependencies.deps for j in jobs] == [j.dependencies.deps for j in before]
        seen |= set(res.code.tolist())
        assert int(erased.sum()) == int(res.ev_stats[0])
        if name.startswith("repeat"):
            assert int(res.ev_stats[2]) >= 1
        if name == "event_misses":
            assert res.ev_stats.tolist() == [4, 5, 5]
    assert seen == set(range(12))
    rows = {j.job_id: len(j.dependencies.deps) for j in next(c for c in cases if c[0] == "long_lists_lane_0_and_63")[2]}
    assert rows[gc._id(0)] == 65 and rows[gc._id(63)] == 200 and rows[gc._id(127)] == 64
    for n, asc, is_or, want in ((70, True, False, ref.OK), (70, False, False, ref.DEPENDENCY), (70, False, True, ref.DEPENDENCY), (70, True, True, ref.OK)):
        res, _, _ = gc.expected(gc.NOW, *gc.repeats(n, asc, is_or))
        assert int(res.code[1]) == want and int(res.ev_stats[0]) == 2 and int(res.ev_stats[2]) == n - 1
