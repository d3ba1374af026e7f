"""The host refusals of the three features that share one record space (csrc/acct_space_host.inc: the run limits, the submit limits, the
usage tables), reached through the engine on the GPU: for each set call a two-account cycle and too many records by the counts alone
(tables None), for each per-call entry point one key out of range.  Code and message are those of the CPU tables
(tests/test_limits_host.py, tests/test_submit_host.py, tests/test_usage_host.py: the same rules compiled with g++).  Every refusal
comes from the host, in front of any launch; after each one a valid call on the same handle at U = 2, UA = 2, A = 2, Q = 1, Pn = 1 with
3 jobs is held to the feature's oracle or pyref (integers, no tolerance)."""
import numpy as np
import pytest

from cranesched_amd import abi, limits as lm, submit as sb, usage as us
from cranesched_amd.engine import EngineError
from tests import kat
from tests import submit_case as sc
from tests import submit_pyref as sp
from tests import usage_case as uc
from tests import usage_pyref as up
from tests.test_gpu_submit_limits import _same
from tests.test_limits_host import WANT as LIMITS_WANT
from tests.test_run_limits import NOW, _cluster, _gpu_vs_oracle, _limjobs, _tables
from tests.test_submit_host import WANT as SUBMIT_WANT
from tests.test_usage_host import WANT as USAGE_WANT

pytestmark = pytest.mark.gpu
NONE = lm.LIM_NONE
TREE, CYCLE = [NONE, 0], [1, 0]
MANY = 0x80000000     # users: with 2 QoS the user x qos table alone has 2^32 records


def _refused(want, call, *args):
    code, msg = want
    with pytest.raises(EngineError) as e:
        call(*args)
    assert e.value.status == code and str(e.value) == f"{abi.STATUS_STR[code]}: {msg}"


def test_run_limits(engine_default):
    cluster, lay = _cluster()
    jobs = kat.jobs([dict(cpu=1)] * 3)
    ua = [(0, 1), (1, 0)]
    t = _tables([lm.qos_limits(max_jobs_per_user=1)], TREE, 2, ua)
    lj = _limjobs([(0, 0, 0), (1, 0, 0), (1, 0, 0)], ua, jobs.time_limit_sec)
    eng = engine_default(device=0)
    try:
        def valid():
            reason, _ = _gpu_vs_oracle(None, cluster, jobs, NOW, lay, t, lj, "after a refusal", eng=eng)
            assert list(reason) == [0, 0, 3]                   # user 1's second job: QosJobsResourceLimit
        valid()
        _refused(LIMITS_WANT["chain_cycle_of_two"], eng.set_run_limits, _tables([lm.qos_limits()], CYCLE, 2, ua))
        valid()
        _refused(LIMITS_WANT["too_many_records"], eng.set_run_limits, _tables([lm.qos_limits()] * 2, TREE, MANY, ua))
        valid()
        bad = _limjobs([(0, 1, 0), (1, 0, 0), (1, 0, 0)], ua, jobs.time_limit_sec)
        _refused(LIMITS_WANT["qos_out_of_range"], eng.apply_run_limits, bad)
        valid()
    finally:
        eng.close()


def test_submit_limits(engine_default):
    def tables(parent=TREE, U=2, Q=1):
        return sb.SubmitTables(layout=sc.LAYOUT, num_users=U, num_user_accts=2, num_partitions=1,
                               qos=np.array([sb.submit_qos(max_submit_jobs_per_user=1)] * Q), acct_parent=np.array(parent, np.uint32))
    t, jobs = tables(), sc.make_jobs(3)
    keys = sb.SubmitKeys(user=[0, 1, 1], user_acct=[0, 1, 1], account=[1, 0, 0], qos=[0, 0, 0])
    want = sp.run(t, jobs, keys)
    assert list(want[0]) == [abi.SUBMIT_OK, abi.SUBMIT_OK, abi.SUBMIT_MAX_JOB_COUNT_PER_USER]
    eng = engine_default(device=0)
    try:
        def valid():
            eng.set_submit_limits(t)
            _same("after a refusal", eng.check_submissions(jobs, keys), eng.submit_usage(), want)
        valid()
        _refused(SUBMIT_WANT["chain_cycle_of_two"], eng.set_submit_limits, tables(CYCLE))
        valid()
        _refused(SUBMIT_WANT["too_many_records"], eng.set_submit_limits, tables(U=MANY, Q=2))
        valid()
        bad = sb.SubmitKeys(user=[0, 1, 1], user_acct=[0, 1, 1], account=[1, 0, 0], qos=[1, 0, 0])
        _refused(SUBMIT_WANT["qos_out_of_range"], eng.check_submissions, jobs, bad)
        valid()
    finally:
        eng.close()


def test_usage_tables(engine_default):
    t = uc.tables(TREE, U=2, Q=1, Pn=1, value=uc.FIVE, submit=5)
    row = dict(cpu=256, mem=uc.GIB, wall=600, jobs=1, submit=1, names=[1], classes=[1])
    js = uc.rows(dict(user=0, account=1, **row), dict(user=1, account=0, **row), dict(user=1, account=0, **row))
    want, wnf, wof = up.apply(t, t.state(), uc.REL, js)
    eng = engine_default(device=0)
    try:
        def valid():
            eng.set_usage_tables(t)
            nf, of, _ = eng.release_usage(js)
            assert np.array_equal(nf, wnf) and np.array_equal(of, wof) and eng.usage_tables().differences(want) == [], "after a refusal"
        bare = lambda parent, U=2, Q=1: us.UsageTables(layout=uc.LAYOUT, num_users=U, num_user_accts=2, num_qos=Q, num_partitions=1,
                                                       acct_parent=np.array(parent, np.uint32))
        valid()
        _refused(USAGE_WANT["chain_cycle"], eng.set_usage_tables, bare(CYCLE))
        valid()
        _refused(USAGE_WANT["too_many_records"], eng.set_usage_tables, bare(TREE, U=MANY, Q=2))
        valid()
        bad = uc.rows(dict(user=0, account=1, qos=1, **row), dict(user=1, account=0, **row), dict(user=1, account=0, **row))
        _refused(USAGE_WANT["qos_out_of_range"], eng.release_usage, bad)
        valid()
    finally:
        eng.close()
