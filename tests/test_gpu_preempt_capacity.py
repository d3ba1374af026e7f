"""The refusals of cns_select_preempt behind its cycle (cranesched_amd/csrc/preempt_host.inc: fold) on the device: result arrays one entry
short of what the oracle's answer needs, in `capacity`, then `cancel_capacity`, then `preempting_capacity`.  Each is an ordinary status
return with its message; the handle then serves a correctly sized call (held to the oracle) and a plain cycle, which shows the resident
end times were put back behind every refused call.  cranesched_amd/engine.py sizes cns_preempt_out itself, so the calls go through the
C ABI with arrays of exactly the stated lengths."""
import ctypes as C

import numpy as np
import pytest

from cranesched_amd import abi
from tests import preempt_seams as ps
from tests.test_preempt import compare_engine

pytestmark = pytest.mark.gpu

# the smallest seam case whose oracle run cancels at least two running jobs and carries a preempting set (asserted below)
CASE = "ties_mix"
INVALID_ARG = -1   # CNS_ERR_INVALID_ARG (include/crane_gpu/node_select.h)


def call(eng, now, jobs, pre, capacity, cancel_capacity, preempting_capacity):
    """cns_select_preempt with result arrays of exactly these lengths -> (status, message, Placements, PreemptOut)."""
    out = abi.Placements(jobs.num_jobs, jobs.total_places())
    po = abi.PreemptOut(jobs.num_jobs, len(pre.rn_job_id))
    po.capacity, po.preempted = capacity, np.zeros(capacity, np.uint32)
    po.cancelled, po.preempting = np.zeros(cancel_capacity, np.uint32), np.zeros(preempting_capacity, np.uint32)
    cj, co, cp, cpo = jobs.to_c(), out.to_c(), pre.to_c(), po.to_c()
    assert (cpo.capacity, cpo.cancel_capacity, cpo.preempting_capacity) == (capacity, cancel_capacity, preempting_capacity)
    rc = eng._L.cns_select_preempt(eng._h, C.c_int64(now), C.byref(cj), C.byref(cp), C.byref(co), C.byref(cpo))
    msg = eng._L.cns_last_error(eng._h)
    return rc, msg.decode() if msg else "", out, po


def test_short_result_arrays_are_refused_and_the_handle_goes_on(gpu):
    from cranesched_amd import engine
    from oracle import pyoracle
    c, j, now, run, pre = ps.case(engine.preempt_shape(), CASE).inputs
    ref = pyoracle.select(c, j, now, running=run, preempt=pre)
    pairs, cancelled, preempting = sum(len(x) for x in ref.preempt_out.lists()), ref.preempt_out.cancelled_ids(), ref.preempt_out.preempting_ids()
    assert len(cancelled) >= 2 and len(pre.preempting) and len(preempting) > len(cancelled), "conditions on the inputs"
    eng = engine.GpuNodeSelector(device=0)
    try:
        eng.set_nodes(c)
        eng.set_running(run)
        for short, text in (((pairs - 1, len(cancelled), len(preempting)), "cns_preempt_out::capacity too small"),
                            ((pairs, len(cancelled) - 1, len(preempting)), "cancel_capacity too small"),
                            ((pairs, len(cancelled), len(preempting) - 1), "preempting_capacity too small")):
            rc, msg, _, _ = call(eng, now, j, pre, *short)
            assert (rc, msg) == (INVALID_ARG, "cns_select_preempt: " + text), (short, rc, msg)
        rc, msg, pl, po = call(eng, now, j, pre, pairs, len(cancelled), len(preempting))   # exactly what the answer needs
        assert rc == 0, msg
        compare_engine(CASE, c, j, ref, eng, pl, po)
        plain = pyoracle.select(c, j, now, running=run)
        assert ref.placements.diff(plain.placements) is not None, "a condition on the inputs: preemption changes the cycle"
        d = eng.node_select(now, j).diff(plain.placements)
        assert d is None, f"the plain cycle behind the calls differs from the oracle: {d}"
    finally:
        eng.close()
