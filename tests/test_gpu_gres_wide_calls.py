"""The calls merged after tests/test_gpu_gres_wide.py, on its layouts (tests/gres_wide.py: a 64-slot class with bit 63, eight classes
under four names with class index and bit position disagreeing, uneven widths, random layouts): cns_probe, cns_validate_jobs,
cns_check_submissions, and the device ledger with its attribute columns and its cycle with preemption.  Each against the truth its own
test file uses — tests/probe_case.expected, tests/valid_pyref.py, tests/submit_pyref.py, tests/running_pyref.py with the oracle and a
second engine fed by cns_set_running — for equality.  tests/test_gres_wide.py asserts, on those references' answers, that the cases
reach the edges they are for: saturated 4-bit counts under the probes, request bytes decided by the clamp to 65, codes that depend on
CheckGres_'s walk order, ledger words above bit 31.

The expected answers are computed once per case and shared."""
import functools

import numpy as np
import pytest

from cranesched_amd import abi
from oracle import pyoracle
from tests import gres_wide as gw
from tests import probe_case as pc
from tests import running_case as rc
from tests import running_pyref as rp
from tests import submit_case as sc
from tests import submit_pyref as sp
from tests import valid_case as vc
from tests import valid_pyref

pytestmark = pytest.mark.gpu

LAYOUTS = gw.NAMED + [3, 5]
SUBMIT_LAYOUTS = ["eight_by_8_four_names", "uneven", 3, 5]


# ---- cns_probe ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probe_scenario(name):
    """-> (cluster, jobs, probes, now, running, reservations, expected)"""
    rv = None
    if name == "shared":          # the same nodes in 4 partitions that share them; the probes go to all four
        c, j, p, now, run = gw.probe_case(1, "uneven")
        c2, j = gw.repartition(c, j, 1, "all+subsets")
        _, p = gw.repartition(c, p, 1, "all+subsets")
        c = c2
    elif name == "resv":          # reservations that hold big-class slots; a quarter of the probes run inside one
        c, j, now, run, rv = gw.resv_case(50, layout="uneven")
        p = pc.take(j, np.arange(32))
    else:
        c, j, p, now, run = gw.probe_case(1, name)
    return c, j, p, now, run, rv, pc.expected(c, j, p, now, running=run, reservations=rv)


def _probe_parity(cls, name):
    from tests.test_gpu_probe import _assert_probes, _cycle
    c, j, p, now, run, rv, exp = _probe_scenario(name)
    eng, got_cycle = _cycle(cls, c, j, now, run, rv, {})
    try:
        # the cycle itself is the oracle's (else a probe mismatch would say nothing about the probe path)
        ref = pyoracle.select(c, j, now, running=run, reservations=rv)
        assert got_cycle.diff(ref.placements) is None, f"{name}: the cycle differs from the oracle"
        _assert_probes(f"wide GRES {name} behind {eng.last_kernel()}", eng.probe(p), exp, p)
    finally:
        eng.close()


@pytest.mark.parametrize("lay", LAYOUTS)
def test_probes(engine_cls, lay):
    _probe_parity(engine_cls, lay)


@pytest.mark.parametrize("name", ["shared", "resv"])
def test_probes_on_shared_nodes_and_reservations(engine_default, name):
    c, j, p, now, run, rv, exp = _probe_scenario(name)
    m = pc.outcome_mix(exp, p, now)     # (asserted on the oracle's answers)
    assert m["now"] + m["later"] >= 8 and (name != "shared" or len(set(p.partition.tolist())) >= 4), m
    assert name != "resv" or (p.reservation != abi.RESV_NONE).sum() >= 3
    _probe_parity(engine_default, name)


@pytest.mark.parametrize("kind", gw.DIP_KATS)
def test_probe_behind_a_saturated_dip(engine_cls, kind):
    """gw.probe_dip_kat: the probes' window reaches a dip whose 4-bit class count saturates (24 free slots); by hand and by the oracle
    they start now on that node."""
    from tests.test_gpu_probe import _assert_probes, _cycle
    c, j, rv, p, now, free, want = gw.probe_dip_kat(kind)
    exp = pc.expected(c, j, p, now, reservations=rv)
    eng, got_cycle = _cycle(engine_cls, c, j, now, None, rv, {})
    try:
        assert got_cycle.diff(pyoracle.select(c, j, now, reservations=rv).placements) is None, "the cycle differs from the oracle"
        got = eng.probe(p)
        _assert_probes(f"saturated dip ({kind}) behind {eng.last_kernel()}", got, exp, p)
        assert [(int(got.start_sec[i]), int(got.node_idx[int(got.place_offsets[i])])) for i in range(3)] == want
    finally:
        eng.close()


# ---- cns_validate_jobs -------------------------------------------------------------------------------------------------------------
def _validate(engine_default, what, cl, jobs, want_code, want_elig):
    from tests.test_gpu_validity import _same
    eng = engine_default(device=0)
    try:
        eng.set_nodes(cl)
        _same(what, eng.validate_jobs(jobs), want_code, want_elig)
    finally:
        eng.close()


@pytest.mark.parametrize("table", ["one64", "eight_by_8_four_names", "mem_2pow63"])
def test_validity_hand_tables(engine_default, table):
    """By hand, not from the restatement (tests/test_valid_pyref.py holds the restatement to the same rows)."""
    cl, jobs, want_code, want_elig, _ = vc.hand_wide()[table]
    _validate(engine_default, f"hand table {table}", cl, jobs, want_code, want_elig)


@pytest.mark.parametrize("lay", LAYOUTS)
def test_validity_of_the_wide_queues(engine_default, lay):
    c, j, now, run = gw.gres_wide_case(1, N=96, J=700, P=2, running=60, layout=lay)
    _validate(engine_default, f"wide GRES {lay}", c, j, *valid_pyref.check(c, j, None))


# ---- cns_check_submissions ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _submit(lay):
    t, jobs, keys = gw.submit_case(11, lay)
    return t, jobs, keys, sp.run(t, jobs, keys)


@pytest.mark.parametrize("mode", ["rounds", "seq"])
def test_submit_hand_table(engine_default, monkeypatch, mode):
    from tests.test_gpu_submit_limits import _mode, _run
    _mode(monkeypatch, mode)
    t, jobs, keys, codes = sc.hand_table_wide()
    want = sp.run(t, jobs, keys)
    assert np.array_equal(want[0], codes)       # (tests/test_submit_pyref.py; the codes below are the hand-derived ones)
    _run(engine_default, t, jobs, keys, (codes,) + want[1:], "hand table on eight_by_8_four_names")


@pytest.mark.parametrize("mode", ["rounds", "seq"])
@pytest.mark.parametrize("lay", SUBMIT_LAYOUTS)
def test_submit_limits(engine_default, monkeypatch, lay, mode):
    from tests.test_gpu_submit_limits import _mode, _run
    _mode(monkeypatch, mode)
    t, jobs, keys, want = _submit(lay)
    _run(engine_default, t, jobs, keys, want, f"wide GRES {lay} {mode}")


# ---- the device ledger -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ledger_scenario(lay):
    return rc.scenario(3, case=gw.wide_case_of(lay))


@pytest.mark.parametrize("lay", gw.NAMED)
def test_ledger_four_consecutive_cycles(engine_cls, lay):
    """tests/running_case.scenario over a wide layout, replayed as tests/test_gpu_running.py replays its own: after every call the
    ledger against running_pyref, every cycle against the oracle and against a second engine fed by cns_set_running."""
    from tests.test_gpu_running import Trio
    cluster, first, cycles = _ledger_scenario(lay)
    t = Trio(engine_cls, cluster)
    try:
        t.seed(first)
        for i, c in enumerate(cycles):
            t.same_ledger(c.before, f"{lay} cycle {i}: before")
            pl = t.cycle(c.before, c.now, c.jobs, f"{lay} cycle {i}")
            assert pl.diff(c.oracle.placements) is None
            led = c.before.copy()
            nret, nadm = t.advance(led, c.retire, c.now, c.jobs, pl, c.job_ids, admit=c.admit, tag=f"{lay} boundary {i}")
            assert (nret, nadm) == (c.num_retired, c.num_admitted) and nadm >= 10 and nret >= 1
            t.same_ledger(c.after, f"{lay} cycle {i}: after")
    finally:
        t.close()


def test_ledger_attribute_columns(engine_default):
    """cns_running_seed_attrs / cns_running_advance_attrs on the eight_by_8_four_names scenario: the columns against
    tests/running_attrs_pyref.py, the ledger against the plain calls' and pyref's."""
    from tests.test_gpu_running_attrs import Pair
    cluster, first, cycles = _ledger_scenario("eight_by_8_four_names")
    p = Pair(engine_default, cluster, first.copy())
    try:
        for i, c in enumerate(cycles):
            pl = p.cycle(c.now, c.jobs)
            assert pl.diff(c.oracle.placements) is None
            nret, nadm = p.advance(c.retire, c.now, c.jobs, c.oracle.placements, c.job_ids, admit=c.admit, tag=f"boundary {i}")
            assert (nret, nadm) == (c.num_retired, c.num_admitted)
            assert rp.same_ledger(p.ref.ledger.arrays(), c.after.arrays()) is None
    finally:
        p.close()


def test_ledger_cycle_with_preemption(gpu):
    """One cns_running_select_preempt on a ledger whose rows hold big-class slots (a preemption releases 16 and more slots of a class at
    once): against cns_set_running + cns_select_preempt on a second engine, the oracle, and the index of running_preempt_pyref."""
    from tests.test_gpu_running_preempt import check_case
    c, j, now, run, pre = gw.preempt_case(60, N=24, J=400, P=2, running=120, layout="uneven")
    assert any(int(g) >> 32 for g in run.alloc_gres) and any(int(g) >> 63 for g in run.alloc_gres), "a condition on the inputs: ledger words above bit 31"
    eng, (pl, po), ref = check_case("wide GRES uneven", c, j, now, run, pre)
    try:
        assert sum(len(x) for x in po.lists()) > 0, "a condition on the inputs: the queue preempts"
    finally:
        eng.close(); ref.close()
