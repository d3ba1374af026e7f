"""The HIP step scheduler (k_sched_steps through cns_schedule_steps) on the edge families of tests/steps_edge.py, bit for bit against the
oracle: every field of StepResults, so also the CNS_NODE_NONE / zero fill of what pending steps own and step_res_avail_ afterwards; against
the reference's own compiled SchedulePendingSteps too where oracle/_ref came with the tree.  tests/test_steps_edge.py shows on the CPU that
the cases reach their edges.  No input here is one the host pass ought to refuse: those are tests/test_steps_host.py's, on the CPU."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import kat, steps_edge as se
from tests.test_steps_edge import oracle_case

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    d = got.diff(want)
    assert d is None, f"{what}: {d}"


@pytest.mark.parametrize("name", list(se.CASES))
def test_gpu_edge_case(engine_default, name):
    lay, jobs, steps, ref = oracle_case(name)
    eng = engine_default(device=0)
    try:
        eng.set_nodes(kat.cluster([4], layout=lay))      # the handle's GRES layout comes with a node table
        got, _ = eng.schedule_steps(jobs, steps)
    finally:
        eng.close()
    _same(got, ref, "engine vs oracle")
    if pyoracle.ref_available():
        _same(got, pyoracle.schedule_steps(lay, jobs, steps, backend="ref"), "engine vs the reference's own code")


def test_gpu_buffers_reused_across_calls_of_different_sizes(engine_default):
    """One handle: a deep_heap case, one job, no job, the first case again (the d_step buffers shrink in use, never in size), and the
    cycle's resident state before and after."""
    big, one, none = (oracle_case(n) for n in (f"deep_heap-{se.DEEP_HEAP_SEEDS[0]}", "launch-1", "launch-0"))
    lay = big[0]
    cluster = kat.cluster([4, 4, 8, 8], layout=lay)
    sel_jobs = kat.jobs([dict(cpu=2), dict(cpu=4, k=2, ntasks=4), dict(cpu=1, ntasks=3, tmax=3), dict(cpu=8, k=3, ntasks=3)])
    eng = engine_default(device=0)
    try:
        eng.set_nodes(cluster)
        before = eng.node_select(kat.NOW, sel_jobs)
        d = before.diff(pyoracle.select(cluster, sel_jobs, kat.NOW).placements)
        assert d is None, d
        results = []
        for lay_c, jobs, steps, ref in (big, one, none, big):
            got, _ = eng.schedule_steps(jobs, steps)
            _same(got, ref, f"call {len(results)}")
            results.append(got)
        for f in results[0].FIELDS:
            assert np.array_equal(getattr(results[0], f), getattr(results[3], f)), f
        after = eng.node_select(kat.NOW, sel_jobs)
        assert after.diff(before) is None, after.diff(before)
    finally:
        eng.close()
