"""The seam cases of the serial protocol (tests/serial_seams.py; tests/test_serial_seams.py asserts on the CPU that each one sits on its
seam) on the engine: placements, reasons, starts, the fp64 costs as bit patterns (helpers.assert_same) and the final time map of every
seam node, entry for entry, must equal the oracle's — twice on one handle, the second cycle equal to the first (family Q: three
different cycles on one handle, each held to the oracle on its own).  last_kernel() must start with k_giant and name the helper count
the plan rule predicts, or start with k_mem and not name the giant instantiation: a silent fall-back to the other path fails.  The
replays of the select suite run as one test per (select family, instantiation), which names every case whose answers differ; an engine
error or a device fault ends such a test at once.  No tolerances: everything is integer or bit-exact.

With the change come the six-cycle controller loop of tests/loop_case.py (without preemption) under `giant`, and the probe families
R-A / R-C of tests/probe_seams.py behind a `giant` cycle.  The serial mode posts NO dips of refused queue jobs: record_dip's callers are
both in wide_test_task, which the serial-only mode never runs (its exact test is k_select's worker_job_slow) — so behind `giant` a probe
reads the dips k_init_nodes posted and nothing else, and check_dip asserts a reservation's dip only."""
import numpy as np
import pytest

from tests import helpers
from tests import loop_case as lc
from tests import serial_seams as sr
from tests.test_gpu_loop import _run as run_loop
from tests.test_gpu_probe_seams import POSTS_QUEUE_DIPS, engines, expected_of, run_family   # noqa: F401 (the two fixtures of that module)
from tests.test_gpu_select_seams import FIELDS

pytestmark = pytest.mark.gpu
SHAPE = sr.SHIPPED


@pytest.fixture(scope="module")
def oracle_of(built):
    """case -> the oracle's run: computed when asked for; the large clusters are used once and not kept."""
    from cranesched_amd import engine
    from oracle import pyoracle
    assert engine.serial_shape() == SHAPE

    def get(case):
        return pyoracle.select(case.cluster, case.jobs, case.now, running=case.running, **case.cfg)
    return get


def same_as_oracle(eng, got, ref, case, tag):
    if case.whole:
        helpers.assert_same(eng, got, ref, case.cluster, tag=tag)
    else:                                # (the oracle builds no node of a partition without a job: the placements and the busy partitions' costs)
        d = got.diff(ref.placements)
        assert d is None, f"{tag}: placements differ from the oracle at {d}"
        off = case.cluster.part_offsets
        gc, rc = eng.costs().view(np.uint64), ref.costs().view(np.uint64)
        for p in sorted({int(x) for x in case.jobs.partition}):
            lo, hi = int(off[p]), int(off[p + 1])
            assert np.array_equal(gc[lo:hi], rc[lo:hi]), f"{tag}: fp64 costs of partition {p} differ"
    for n in case.nodes:
        a, b = eng.timeline(int(n)), ref.timeline(int(n))
        for f in FIELDS:
            assert np.array_equal(a[f], b[f]), f"{tag}: time map of node {n} differs in {f}:\n{a[f]}\n{b[f]}"


def check_kernel(eng, case):
    k = eng.last_kernel()
    head, nh = case.kernel[1]
    assert k.startswith(head), (case.name, k, case.kernel)
    if head == "k_giant":
        assert f"+ {nh} helper workgroups per partition" in k and f" on {case.busy} group(s)" in k, (case.name, k, case.kernel)
    elif head == "k_mem":
        assert "giant" not in k and f" on {case.busy} group(s)" in k, (case.name, k, case.kernel)


def run_case(eng, case, ref, monkeypatch, again=True):
    if case.kernel[0] is None:
        monkeypatch.delenv("CNS_SELECT_KERNEL", raising=False)
    else:
        monkeypatch.setenv("CNS_SELECT_KERNEL", case.kernel[0])
    eng.set_nodes(case.cluster)
    eng.set_running(case.running)
    first = eng.node_select(case.now, case.jobs)
    same_as_oracle(eng, first, ref, case, case.name)
    check_kernel(eng, case)
    if again:
        second = eng.node_select(case.now, case.jobs)
        assert first.diff(second) is None, f"{case.name}: the second cycle on the handle differs from the first"
        same_as_oracle(eng, second, ref, case, case.name + ", again")
        check_kernel(eng, case)


@pytest.mark.parametrize("family,name", [(f, n) for f in ("N", "H", "W", "G", "P") for n in sr.case_names(SHAPE, f)])
def test_seam(engine_default, engines, oracle_of, monkeypatch, family, name):
    case = sr.case(SHAPE, family, name)
    run_case(engines(case.cfg), case, oracle_of(case), monkeypatch)


def test_three_cycles_on_one_handle(engine_default, engines, oracle_of, monkeypatch):
    """Family Q: another queue on the same snapshot, then another cluster with another helper count, each cycle compared on its own."""
    q = sr.case(SHAPE, "Q", "three_cycles")
    eng = engines({})
    for link in q.chain:
        run_case(eng, link, oracle_of(link), monkeypatch, again=False)


@pytest.mark.parametrize("family", sr.R_FAMILIES)
def test_replayed_select_seams(engine_default, engines, oracle_of, monkeypatch, family):
    """Every case of a select family under `giant`, unpadded (k_giant) or padded to 17 busy partitions (k_mem), in one test.  A case
    whose answers differ (AssertionError) is written down and the next one runs; anything else — an error of the engine, a device
    fault, a failed launch — ends the test at once: nothing more is started on the device behind it."""
    failed = []
    names = sr.case_names(SHAPE, family)
    for name in names:
        case = sr.case(SHAPE, family, name)
        try:
            run_case(engines(case.cfg), case, oracle_of(case), monkeypatch)
        except AssertionError as e:
            failed.append(f"{name}: {e}")
    assert not failed, f"{len(failed)} of {len(names)} cases of {family} fail:\n" + "\n".join(failed)


def test_the_controller_loop_under_giant(engine_default, monkeypatch):
    """tests/loop_case.py's six cycles on one handle, without preemption, every partition and every reservation's virtual partition on k_giant."""
    monkeypatch.setenv("CNS_SELECT_KERNEL", "giant")
    scen = lc.scenario(1)
    served = []

    def hook(loop, i, step):
        if step == "d":                  # behind the cycle of step c
            served.append(loop.eng.last_kernel())
    assert len(run_loop(engine_default, scen, hook=hook)) > 6 * len(scen[4])
    assert len(served) == len(scen[4]) and all(k.startswith(("k_giant", "k_mem", "none")) for k in served), served
    assert any(k.startswith("k_giant") for k in served), served


@pytest.mark.parametrize("family", ("RA", "RC"))
def test_probes_behind_a_giant_cycle(engine_default, engines, expected_of, monkeypatch, family):
    assert "giant" not in POSTS_QUEUE_DIPS, "the serial mode posts no dip of a refused queue job (see the module docstring)"
    monkeypatch.setenv("CNS_SELECT_KERNEL", "giant")
    run_family(engines, expected_of, family, "giant")
