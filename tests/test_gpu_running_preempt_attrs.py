"""cns_running_select_preempt_attrs (include/crane_gpu_running/running_attrs.h): the cycle with preemption that reads the running
jobs' qos, qos_priority and start_sec from the ledger's columns, against cns_running_select_preempt on a second engine that is fed the
downloaded columns (running_attrs() and the ids of running_ledger()) — on the scenarios of tests/test_gpu_running_preempt.py, imported
from there.  Compared without a tolerance: placements, reasons and start times, the preempted lists, the cancelled ids, the preempting
set, and every field of preempt_index()."""
import ctypes as C

import numpy as np
import pytest

from cranesched_amd import abi
from tests import kat_preempt
from tests import test_gpu_running_preempt as trp
from tests.test_preempt import overlap_preempt_case, random_preempt_case, resv_preempt_case

pytestmark = pytest.mark.gpu


def attrs_of(pre, n=None):
    """The running side of a Preempt as the columns of a seed (partition priority and account do not matter to a cycle)."""
    n = len(pre.rn_job_id) if n is None else n
    return abi.RunningAttrs(qos=pre.rn_qos, qos_priority=pre.rn_qos_priority, partition_priority=np.arange(n) % 3, account=np.arange(n) % 2, start_sec=pre.rn_start_sec)


def with_running_side(pre, ids, qos, qprio, start, preempting=None):
    return abi.Preempt(pre.qos_preempt, pre.pd_job_id, pre.pd_qos, pre.pd_qos_priority, pre.pd_priority, ids, qos, qprio, start,
                       preempting=list(pre.preempting if preempting is None else preempting), enabled=pre.enabled)


def bare(pre, preempting=None):
    return with_running_side(pre, [], [], [], [], preempting)


def fed_from(eng, pre, preempting=None):
    """What a caller of cns_running_select_preempt would hand in, taken from the device."""
    cols, ids = eng.running_attrs(), eng.running_ledger()[1]
    return with_running_side(pre, ids, cols["qos"], cols["qos_priority"], cols["start_sec"], preempting)


def attrs_engine(c, run, pre, resv=None):
    from cranesched_amd.engine import GpuNodeSelector
    eng = GpuNodeSelector(device=0)
    eng.set_nodes(c)
    if resv is not None:
        eng.set_reservations(resv)
    none = run is None or len(run.end_sec) == 0
    eng.seed_running(None if none else run, pre.rn_job_id, attrs=attrs_of(pre))
    return eng


def same_index(tag, a, b):
    x, y = a.preempt_index(), b.preempt_index()
    for f in x:
        assert np.array_equal(x[f], y[f]), f"{tag}: preempt_index differs in {f}"


def check_case(tag, c, j, now, run, pre, resv=None):
    a = attrs_engine(c, run, pre, resv)
    b = trp.resident_engine(c, run, pre.rn_job_id, resv)
    try:
        fed = fed_from(a, pre)
        assert np.array_equal(fed.rn_job_id, pre.rn_job_id) and np.array_equal(fed.rn_qos, pre.rn_qos) and np.array_equal(fed.rn_start_sec, pre.rn_start_sec)
        ra = a.node_select_preempt_resident(now, j, bare(pre), from_attrs=True)
        rb = b.node_select_preempt_resident(now, j, fed)
        trp.same_results(tag, ra, rb)
        assert a.last_kernel().split(" [")[0] == b.last_kernel().split(" [")[0]
        same_index(tag, a, b)
    except BaseException:
        a.close(); b.close()
        raise
    return a, ra, b


@pytest.mark.parametrize("scn", kat_preempt.scenarios(), ids=lambda s: s[0])
def test_known_answers(gpu, scn):
    name, c, j, r, pre, expect = scn
    a, (pl, po), b = check_case(name, c, j, kat_preempt.NOW, r, pre)
    try:
        assert po.cancelled_ids() == expect["cancelled"] and po.preempting_ids() == expect["preempting"]
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("seed", range(6))
def test_random_cases(gpu, seed):
    c, j, now, run, pre = random_preempt_case(500 + seed, N=6 + seed % 7, J=50 + seed % 40, P=1 + seed % 2, running=10 + seed % 11)
    a, (pl, po), b = check_case(f"random {seed}", c, j, now, run, pre)
    a.close(); b.close()


def test_the_known_answers_preempt_running_jobs():
    """A condition on the inputs: ledger rows are preempted, so their ids are picked on the device."""
    assert sum(len(s[5]["cancelled"]) for s in kat_preempt.scenarios()) >= 2


@pytest.mark.parametrize("seed", range(2))
def test_rows_inside_reservations(gpu, seed):
    c, j, now, run, rv, pre = resv_preempt_case(seed)
    a, _, b = check_case(f"resv {seed}", c, j, now, run, pre, resv=rv)
    a.close(); b.close()


@pytest.mark.parametrize("seed,lay", [(0, "all+subsets"), (1, "chain")])
def test_partitions_that_share_nodes(gpu, seed, lay):
    c, j, now, run, pre = overlap_preempt_case(seed, layout=lay)
    a, _, b = check_case(f"overlap {seed} {lay}", c, j, now, run, pre)
    a.close(); b.close()


def test_a_ledger_around_a_workgroup_and_of_zero_rows(gpu):
    for R in (0, 257):
        led = trp.ledger_of(5, [1] * R)
        jobs = trp.tiny_queue(128 - R // 5 + 1 if R else 128)   # one core more than the emptiest node has free
        pre = trp.tiny_preempt(led, jobs, [led.ids()[0], 4242] if R else [4242])
        run, _ = led.arrays()
        a, (pl, po), b = check_case(f"{R} rows", trp.flat_cluster(5), jobs, trp.NOW, run if R else None, pre)
        assert (sum(len(x) for x in po.lists()) > 0) == (R > 0)
        a.close(); b.close()


def test_disabled_is_the_plain_cycle(gpu):
    c, j, now, run, pre = trp._case4()
    a = attrs_engine(c, run, pre)
    b = trp.resident_engine(c, run, pre.rn_job_id)
    try:
        off = with_running_side(pre, pre.rn_job_id, pre.rn_qos, pre.rn_qos_priority, pre.rn_start_sec)
        off.enabled = False
        ra = a.node_select_preempt_resident(now, j, off, from_attrs=True)
        trp.same_results("disabled", ra, b.node_select_preempt_resident(now, j, off))
        assert ra[0].diff(b.node_select(now, j)) is None
    finally:
        a.close(); b.close()


def _raw(eng, now, jobs, pre, keep):
    """The C call with the rn_* pointers of `keep` left in place."""
    out, pout = abi.Placements(jobs.num_jobs, jobs.total_places()), abi.PreemptOut(jobs.num_jobs, len(pre.rn_job_id))
    cj, co, cp, cpo = jobs.to_c(), out.to_c(), pre.to_c(), pout.to_c()
    for f in ("rn_job_id", "rn_qos", "rn_qos_priority", "rn_start_sec"):
        if f not in keep:
            setattr(cp, f, None)
    rc = eng._L.cns_running_select_preempt_attrs(eng._h, C.c_int64(now), C.byref(cj), C.byref(cp), C.byref(co), C.byref(cpo))
    return rc, eng._L.cns_last_error(eng._h).decode()


def test_a_running_job_array_is_refused_and_a_ledger_without_columns_too(gpu):
    c, j, now, run, pre = trp._case4()
    a = attrs_engine(c, run, pre)
    try:
        before = a.node_select(now, j)
        for f in ("rn_job_id", "rn_qos", "rn_qos_priority", "rn_start_sec"):
            rc, msg = _raw(a, now, j, pre, (f,))
            assert rc == -1 and "must be NULL" in msg, (f, msg)
        assert a.download().diff(before) is None, "no cycle has run"
        rc, msg = _raw(a, now, j, pre, ())
        assert rc == 0, msg
        a.seed_running(run, pre.rn_job_id)
        rc, msg = _raw(a, now, j, pre, ())
        assert rc == -5 and "carries no attribute columns" in msg
    finally:
        a.close()


def test_three_consecutive_cycles_with_the_admit_step_behind_them(gpu):
    """tests/test_gpu_running_preempt.py: test_three_consecutive_cycles, with the columns on the ledger: cycle c from the columns, then
    cns_running_advance_attrs with retire_ids = the cancelled ids and admit = the jobs that started without preempting a running job —
    without the mask it is refused, as behind cns_running_select_preempt.  The second engine makes the plain calls and is fed the
    downloaded columns."""
    c, j, now, run, pre = random_preempt_case(503, N=10, J=60, P=2, running=14)
    J = j.num_jobs
    a = attrs_engine(c, run, pre)
    b = trp.resident_engine(c, run, pre.rn_job_id)
    try:
        preempting, preempted_any = list(pre.preempting), 0
        for cyc in range(3):
            t = now + 60 * cyc
            fed = fed_from(a, pre, preempting)
            assert np.array_equal(fed.rn_job_id, b.running_ledger()[1])
            pl, po = a.node_select_preempt_resident(t, j, bare(pre, preempting), from_attrs=True)
            trp.same_results(f"cycle {cyc}", (pl, po), b.node_select_preempt_resident(t, j, fed))
            same_index(f"cycle {cyc}", a, b)
            lists = po.lists()
            preempted_any += sum(1 for x in lists for pending, _ in x if not pending)
            admit = np.array([int(pl.reason[x]) == 0 and int(pl.start_sec[x]) == t and not any(not pending for pending, _ in lists[x]) for x in range(J)], np.uint8)
            job_ids = 50000 + 1000 * cyc + np.arange(J)
            qa = abi.RunningAttrs(qos=pre.pd_qos, qos_priority=pre.pd_qos_priority, partition_priority=np.zeros(J), account=np.zeros(J))
            assert "missing array: admit" in trp._raises(-1, a.advance_running, po.cancelled_ids(), t, job_ids, attrs=qa)
            got = a.advance_running(po.cancelled_ids(), t, job_ids, admit, attrs=qa)
            want = b.advance_running(po.cancelled_ids(), t, job_ids, admit)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and got[2] == int(admit.sum())
            cols = a.running_attrs()
            n = got[2]
            assert list(cols["start_sec"][len(cols["start_sec"]) - n:]) == [t] * n and list(cols["qos"][len(cols["qos"]) - n:]) == list(pre.pd_qos[admit != 0])
            preempting = po.preempting_ids()
        assert preempted_any > 0, "a condition on the inputs: the cycles preempt running jobs"
    finally:
        a.close(); b.close()
