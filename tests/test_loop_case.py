"""tests/loop_case.py held to its conditions on the CPU: what the composed reference must contain for tests/test_gpu_loop.py to show
anything, and that every hand-off of the loop decides a later expected output (a hand-off lost on the device could not pass).
Conditions on the inputs, not measurements: the seed and the sizes of tests/loop_case.py were chosen until they hold."""
import numpy as np
import pytest

from cranesched_amd import abi
from tests import gate_pyref
from tests import loop_case as lc

SEED = 1
NO_RETIRE = [i for i, p in enumerate(lc.PLAN) if p["step"] == 1]
HOLD_ALL = [i for i, p in enumerate(lc.PLAN) if p.get("hold_all")]


@pytest.fixture(scope="module")
def plain(built):
    return lc.scenario(SEED)


@pytest.fixture(scope="module")
def preempting(built):
    return lc.scenario(SEED, preempt=True)


def _mix(c):
    J, pl = c.jobs.num_jobs, c.oracle.placements
    r, s = pl.reason[:J], pl.start_sec[:J]
    return int(((r == 0) & (s == c.now)).sum()), int((s > c.now).sum()), int(((r != 0) & (s == 0)).sum())


@pytest.mark.parametrize("which", ["plain", "preempting"])
def test_conditions(request, which):
    U, resv, first, tables, cycles = request.getfixturevalue(which)
    chunk = max(lc.shapes())
    assert 5 <= len(cycles) <= 6 and 48 <= U.cluster.num_nodes <= 64 and len(first.rows) >= 30
    # the gate: every code
    seen = set(int(x) for c in cycles for x in c.gate.code)
    assert {gate_pyref.HELD, gate_pyref.BEGIN_TIME, gate_pyref.DEPENDENCY, gate_pyref.DEPENDENCY_NEVER, gate_pyref.OK} <= seen
    assert sum(int(c.gate.ev_stats[0]) for c in cycles) > 5, "dependency events of jobs that ended are applied"
    # the queue lengths move both ways across the workgroup's seam
    J = [c.jobs.num_jobs for c in cycles]
    assert any(J[i] > max(J[:i]) and J[i] > chunk > J[i - 1] for i in range(1, len(J))), J
    assert any(0 < J[i] < J[i - 1] / 2 and J[i] < chunk < J[i - 1] for i in range(1, len(J))), J
    assert [i for i, n in enumerate(J) if n == 0] == HOLD_ALL and all(len(cycles[i].pending_ids) > 0 and cycles[i].num_retired > 0 for i in HOLD_ALL)
    P = [len(c.pending_ids) for c in cycles]
    assert min(P) < chunk < max(P), P
    # the order
    assert sum(1 for c in cycles if not np.array_equal(c.order, np.arange(len(c.order)))) >= 3
    # the cycle
    for i, c in enumerate(cycles):
        if c.jobs.num_jobs:
            assert min(_mix(c)) > 0, (i, _mix(c))
    # the codes and the run limits
    other = lambda c: int(np.isin(c.code, (abi.COMMIT_OK, abi.COMMIT_NOT_STARTED), invert=True).sum())
    assert sum(1 for c in cycles if other(c)) >= 2
    assert len({int(x) for c in cycles for x in c.code}) >= 5
    assert sum(1 for c in cycles if np.isin(c.limit_reason, (0, 255), invert=True).any()) >= 2
    assert sum(int(((c.limit_reason == 0) & np.isin(c.blind_reason, (0, 255), invert=True)).sum()) for c in cycles) >= 1, "admitted only because an earlier job was skipped"
    assert sum(1 for c in cycles if c.num_admitted >= 5) >= 3
    # the boundary
    assert len(NO_RETIRE) == 1
    for i, c in enumerate(cycles):
        assert (c.num_retired == 0 and len(c.retire) == 0) if i in NO_RETIRE else c.num_retired >= 1, i
        assert c.num_admitted == int(((c.limit_reason == 0)).sum()) if c.jobs.num_jobs else c.num_admitted == 0
    rows = [r for c in cycles for r in c.after.ledger.rows]
    assert any(r.reservation == 0 and r.job_id >= 2000 for r in rows), "an admitted row inside the reservation"
    assert any(a[0] in U.shared for r in rows if r.job_id >= 2000 for a in r.allocs), "an admitted row on the shared nodes"
    assert any(r.reservation == 0 for r in first.ledger.rows)
    assert len({len(c.after.rows) for c in cycles}) >= 4, "the ledger grows and shrinks"
    # the releases
    assert sum(c.erased for c in cycles) >= 1, "a release that fits a record exactly erases it"
    assert all(len(c.release_ids) + len(c.left_ids) > 0 for i, c in enumerate(cycles) if i not in NO_RETIRE)
    if which == "preempting":
        assert sum(1 for c in cycles if any(not pending for l in c.lists for pending, _ in l)) >= 2, "two cycles preempt a running job"
        assert sum(1 for c in cycles if (c.code == abi.COMMIT_WAITING_PREEMPTION).any()) >= 2
        assert any(c.preempting_in for c in cycles), "a preempting set is passed to the next cycle"
        assert all(c.probes is None for c in cycles)
    else:
        assert all(c.probe_expected is not None for c in cycles)
        r = np.concatenate([c.probe_expected.reason[:lc.PROBES] for c in cycles])
        s = np.concatenate([c.probe_expected.start_sec[:lc.PROBES] - c.now for c in cycles])
        assert ((r == 0) & (s == 0)).any() and (s > 0).any() and ((r != 0) & (s < 0)).any(), "probes that start now, later and never"


# what each hand-off feeds: (the first cycle in which it can show, the steps behind it in that cycle)
BEHIND = {"gate": (0, "bcdefgh"), "order": (0, "cdefgh"), "codes": (0, "efg"), "admitted": (0, "f"), "ledger": (1, "bcdefgh"), "tables": (1, "efg")}


@pytest.mark.parametrize("preempt", [False, True])
@pytest.mark.parametrize("handoff", lc.HANDOFFS)
def test_a_lost_hand_off_changes_a_later_expected_output(request, handoff, preempt):
    """The composed reference recomputed with one hand-off dropped: the consumer's expected output changes in the first cycle in which
    the hand-off carries anything, so a device loop that lost it cannot equal the records."""
    want = request.getfixturevalue("preempting" if preempt else "plain")[4]
    got = lc.scenario(SEED, preempt=preempt, drop=handoff)[4]
    first, steps = BEHIND[handoff]
    for i in range(first):
        assert lc.cycle_key(got[i]) == lc.cycle_key(want[i]), "nothing is dropped before the hand-off carries anything"
    a, b = lc.cycle_key(got[first]), lc.cycle_key(want[first])
    consumer = steps[0]
    assert a[consumer] != b[consumer], f"{handoff}: step {consumer} of cycle {first} does not see the hand-off"
    later = [(i, s) for i in range(first, len(want)) for s in lc.STEPS if (i > first or s in steps[1:]) and lc.cycle_key(got[i])[s] != lc.cycle_key(want[i])[s]]
    assert later, f"{handoff}: nothing behind step {consumer} of cycle {first} changes"


def test_the_scenario_is_the_same_twice(plain):
    again = lc.scenario(SEED)[4]
    assert all(lc.cycle_key(a) == lc.cycle_key(b) for a, b in zip(again, plain[4]))
