"""The submit limits over a batch of submissions (include/crane_gpu_submit/submit_limits.h, csrc/submit_kernels.inc) on the GPU against
tests/submit_pyref.py, the statement-by-statement restatement of AccountMetaContainer.cpp:75-153, :374-506, :694-889: codes, rewritten time
limits, the five count tables, the three exists arrays and num_admitted for equality (all integers, no tolerance).  The hand-derived table,
the seams read from cns_submit_shape, seeded random tables in both modes (the bracketing rounds, and CNS_SUBMIT_MODE=seq: the ordered
single-wave kernel), provable convergence, the domino chain that the rounds do not finish, CNS_SUBMIT_CARRY, independence of the other
calls, and the input rules."""
import functools

import numpy as np
import pytest

from cranesched_amd import abi, submit as sb
from cranesched_amd.engine import EngineError
from tests import submit_case as sc
from tests import submit_pyref as sp

pytestmark = pytest.mark.gpu
MODES = ["rounds", "seq"]


def _mode(monkeypatch, mode):
    if mode == "seq":
        monkeypatch.setenv("CNS_SUBMIT_MODE", "seq")
    else:
        monkeypatch.delenv("CNS_SUBMIT_MODE", raising=False)


def _same(what, got, state, want):
    code, tlo, adm = got
    wcode, wtlo, wadm, wstate = want
    bad = np.flatnonzero(code != wcode)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(wcode)} jobs differ, first job {int(bad[0])}: got "
                           f"{abi.SUBMIT_STR.get(int(code[bad[0]]), int(code[bad[0]]))}, want {abi.SUBMIT_STR[int(wcode[bad[0]])]}")
    assert np.array_equal(tlo, wtlo), f"{what}: rewritten time limits differ"
    assert adm == wadm, f"{what}: {adm} admitted, want {wadm}"
    for f in wstate.__dataclass_fields__:
        assert np.array_equal(getattr(state, f), getattr(wstate, f)), f"{what}: {f} differs"


def _run(engine_default, t, jobs, keys, want=None, what="batch"):
    eng = engine_default(device=0)
    try:
        eng.set_submit_limits(t)
        got = eng.check_submissions(jobs, keys)
        _same(what, got, eng.submit_usage(), want if want is not None else sp.run(t, jobs, keys))
        return eng.submit_timing()
    finally:
        eng.close()


# ---- 1. the hand-derived table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_hand_table(engine_default, monkeypatch, mode):
    _mode(monkeypatch, mode)
    t, jobs, keys, codes, tlo, admitted, created = sc.hand_table()
    want = (codes, tlo, len(admitted), sc.expected_state(t, admitted, created))      # by hand, not from the restatement
    tm = _run(engine_default, t, jobs, keys, want, "hand table")
    assert tm["ordered_fallback"] == (1 if mode == "seq" else 0) and tm["admitted"] == 8
    assert tm["candidates"] == 28 - 9                                                 # jobs 0 - 6, 8 and 9 stop in steps 1 - 9


# ---- 2. seams ------------------------------------------------------------------------------------------------------------------------
def _hot(J, seed=0):
    """Every job on ONE user, account and QoS: each of the 8 table entries they touch is one segment of J items.  Caps in the middle,
    10 % array jobs."""
    r = np.random.default_rng(seed)
    t = sb.SubmitTables(layout=sc.LAYOUT, num_users=1, num_user_accts=1, num_partitions=1,
                        qos=np.array([sb.submit_qos(max_submit_jobs_per_user=max(J // 2, 1) + 40, max_submit_jobs_per_account=max(J // 2, 1) + 20)]),
                        acct_parent=np.array([sb.LIM_NONE], np.uint32))
    count = np.where(r.random(J) < 0.1, r.integers(2, 30, J), 1)
    z = np.zeros(J, np.uint32)
    return t, sc.make_jobs(J), sb.SubmitKeys(z, z, z, z, count)


@pytest.mark.parametrize("mode", MODES)
def test_job_and_item_chunk_seams(engine_default, monkeypatch, mode):
    _mode(monkeypatch, mode)
    eng = engine_default(device=0)
    try:
        c, ic, _ = eng.submit_shape()
        for J in (1, c - 1, c, c + 1, 2 * c + 1, ic - 1, ic + 1):
            t, jobs, keys = _hot(J, seed=J)
            want = sp.run(t, jobs, keys)
            assert J < 4 or 0 < want[2] < J
            eng.set_submit_limits(t)
            _same(f"hot record, J = {J}", eng.check_submissions(jobs, keys), eng.submit_usage(), want)
    finally:
        eng.close()


def test_segment_that_starts_on_the_last_item_of_a_chunk(engine_default, monkeypatch):
    """Sorted by table index the (user, qos) records come first: user 0 holds item_chunk - 1 jobs, so the segment of user 1's record starts
    on the last item of the first chunk and goes on in the second.  Its cap of 2 admits two of user 1's three jobs."""
    _mode(monkeypatch, "rounds")
    eng = engine_default(device=0)
    try:
        _, ic, _ = eng.submit_shape()
        J = ic - 1 + 3
        user = np.array([0] * (ic - 1) + [1, 1, 1], np.uint32)
        t = sb.SubmitTables(layout=sc.LAYOUT, num_users=2, num_user_accts=2, num_partitions=1, qos=np.array([sb.submit_qos(max_submit_jobs_per_user=ic + 1)]),
                            acct_parent=np.array([sb.LIM_NONE], np.uint32), user_qos_submit=np.array([0, ic - 1], np.uint32), user_exists=np.ones(2, np.uint8))
        keys = sb.SubmitKeys(user, user, np.zeros(J, np.uint32), np.zeros(J, np.uint32))
        jobs = sc.make_jobs(J)
        want = sp.run(t, jobs, keys)
        assert want[0][-3:].tolist() == [0, 0, abi.SUBMIT_MAX_JOB_COUNT_PER_USER] and want[2] == J - 1
        eng.set_submit_limits(t)
        _same("segment across a chunk boundary", eng.check_submissions(jobs, keys), eng.submit_usage(), want)
        assert eng.submit_timing()["ordered_fallback"] == 0
    finally:
        eng.close()


# ---- 3. random tables: parity in both modes ------------------------------------------------------------------------------------------------
SIZES = {1: 3000, 2: 20000, 3: 70000}


@functools.lru_cache(maxsize=None)
def _random(seed):
    t, jobs, keys = sc.random_case(seed, SIZES[seed])
    return t, jobs, keys, sp.run(t, jobs, keys)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", sorted(SIZES))
def test_random_tables(engine_default, monkeypatch, seed, mode):
    _mode(monkeypatch, mode)
    t, jobs, keys, want = _random(seed)
    assert len(set(want[0].tolist())) >= 8 and 0 < want[2] < jobs.num_jobs
    tm = _run(engine_default, t, jobs, keys, want, f"seed {seed}")
    print(f"seed {seed}, J = {jobs.num_jobs}, {mode}: rounds {tm['rounds']}, ordered_fallback {tm['ordered_fallback']}, prep {tm['prep_ms']:.3f} ms, "
          f"admit {tm['admit_ms']:.3f} ms")


# ---- 4. provable convergence ---------------------------------------------------------------------------------------------------------------
def test_jobs_on_records_of_their_own_need_two_rounds_at_most(engine_default, monkeypatch):
    _mode(monkeypatch, "rounds")
    J = 300
    i = np.arange(J, dtype=np.uint32)
    t = sb.SubmitTables(layout=sc.LAYOUT, num_users=J, num_user_accts=J, num_partitions=1,
                        qos=np.array([sb.submit_qos(max_submit_jobs=1, deny_on_limit=bool(k % 2), max_jobs_per_user=k % 3) for k in range(J)]),
                        acct_parent=np.full(J, sb.LIM_NONE, np.uint32), user_exists=(i % 2).astype(np.uint8), qos_submit=(i % 5 == 0).astype(np.uint32),
                        qos_exists=np.ones(J, np.uint8))
    tm = _run(engine_default, t, sc.make_jobs(J), sb.SubmitKeys(i, i, i, i), what="own records")
    assert tm["rounds"] <= 2 and tm["ordered_fallback"] == 0


def test_one_record_with_unit_counts_converges(engine_default, monkeypatch):
    _mode(monkeypatch, "rounds")
    J = 1000
    z = np.zeros(J, np.uint32)
    t = sb.SubmitTables(layout=sc.LAYOUT, num_users=1, num_user_accts=1, num_partitions=1, qos=np.array([sb.submit_qos(max_submit_jobs_per_user=J // 3)]),
                        acct_parent=np.array([sb.LIM_NONE], np.uint32))
    tm = _run(engine_default, t, sc.make_jobs(J), sb.SubmitKeys(z, z, z, z), what="one record")
    assert tm["ordered_fallback"] == 0 and tm["admitted"] == J // 3


# ---- 5. the chain the rounds do not finish ---------------------------------------------------------------------------------------------------
def test_domino_chain_falls_back_and_stays_exact(engine_default, monkeypatch):
    _mode(monkeypatch, "rounds")
    eng = engine_default(device=0)
    try:
        n = 2 * eng.submit_shape()[2]
    finally:
        eng.close()
    t, jobs, keys = sc.domino_chain(n)
    want = sp.run(t, jobs, keys)
    assert want[0].tolist() == [0, abi.SUBMIT_MAX_JOB_COUNT_PER_ACCOUNT] * (n // 2)
    tm = _run(engine_default, t, jobs, keys, want, "domino chain")
    assert tm["ordered_fallback"] == 1 and tm["rounds"] == n // 2


# ---- 6. CNS_SUBMIT_CARRY ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_carry(engine_default, monkeypatch, mode):
    _mode(monkeypatch, mode)
    t, jobs, keys, whole = _random(1)
    J, h = jobs.num_jobs, jobs.num_jobs // 2
    ja, ka, jb, kb = sb.slice_jobs(jobs, 0, h), keys.slice(0, h), sb.slice_jobs(jobs, h, J), keys.slice(h, J)
    eng = engine_default(device=0)
    try:
        eng.set_submit_limits(t)
        a = eng.check_submissions(ja, ka)
        b = eng.check_submissions(jb, kb, carry=True)
        _same("two halves, carried", (np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), a[2] + b[2]), eng.submit_usage(), whole)
        # without the flag the second half starts from the tables as set
        _same("second half alone", eng.check_submissions(jb, kb), eng.submit_usage(), sp.run(t, jb, kb))
    finally:
        eng.close()


# ---- 7. independence of the other calls ------------------------------------------------------------------------------------------------------
def test_the_other_calls_do_not_see_it(engine_default):
    """A cycle, cns_validate_jobs and cns_apply_run_limits give identical results with and without cns_check_submissions between them;
    the validity codes are the submit check's `skip`."""
    from cranesched_amd import synth
    cluster, jobs, now = synth.make_config("C1")
    tables, lim_jobs = synth.make_limits("C1", cluster, jobs)
    J = jobs.num_jobs
    r = np.random.default_rng(5)
    st = sb.SubmitTables(layout=cluster.gres, num_users=tables.num_users, num_user_accts=tables.num_user_accts, num_partitions=tables.num_partitions,
                         qos=np.array([sb.submit_qos(max_submit_jobs_per_user=3 + k, deny_on_limit=bool(k % 2)) for k in range(tables.num_qos)]),
                         acct_parent=tables.acct_parent, user_qos=tables.user_qos, acct_qos=tables.acct_qos, qos_usage=tables.qos_usage)
    keys_of = lambda skip: sb.SubmitKeys(lim_jobs.user, lim_jobs.user_acct, lim_jobs.account, lim_jobs.qos, np.where(r.random(J) < 0.1, 7, 1), skip)
    plain, mixed = engine_default(device=0), engine_default(device=0)

    def run_all(eng, check):
        out, sub = {}, []
        eng.set_nodes(cluster)
        eng.set_run_limits(tables)
        if check:
            eng.set_submit_limits(st)
        for step in ("select", "validate", "limits"):
            if step == "select":
                out[step] = eng.node_select(now, jobs)
            elif step == "validate":
                out[step] = eng.validate_jobs(jobs)
            else:
                out[step] = eng.apply_run_limits(lim_jobs) + (eng.usage(),)
            if check:
                skip = (out["validate"][0] != abi.VALID_OK).astype(np.uint8) if "validate" in out else None
                k = keys_of(skip)
                sub.append((eng.check_submissions(jobs, k), eng.submit_usage(), sp.run(st, jobs, k)))
        return out, sub

    try:
        a, _ = run_all(plain, False)
        b, sub = run_all(mixed, True)
        assert b["select"].diff(a["select"]) is None
        assert np.array_equal(b["validate"][0], a["validate"][0]) and np.array_equal(b["validate"][1], a["validate"][1])
        assert np.array_equal(b["limits"][0], a["limits"][0]) and b["limits"][1] == a["limits"][1] and b["limits"][2].same_as(a["limits"][2])
        for i, (got, state, want) in enumerate(sub):
            _same(f"check_submissions number {i} between the other calls", got, state, want)
        assert 0 < sub[-1][2][2] < J
    finally:
        plain.close()
        mixed.close()


# ---- 8. input rules ----------------------------------------------------------------------------------------------------------------------------
def test_input_rules(engine_default):
    t, jobs, keys = sc.random_case(4, 64)
    eng = engine_default(device=0)
    try:
        with pytest.raises(EngineError) as e:
            eng.check_submissions(jobs, keys)
        assert e.value.status == sp.ERR_STATE
        eng.set_submit_limits(t)
        good = eng.check_submissions(jobs, keys)
        state = eng.submit_usage()
        # J == 0 is CNS_OK, writes nothing and leaves the counters
        code, tlo, adm = eng.check_submissions(sb.slice_jobs(jobs, 0, 0), keys.slice(0, 0), carry=True)
        assert len(code) == 0 and adm == 0 and eng.submit_usage().same_as(state)
        # an index out of range: refused on the host, nothing runs; a skipped job's keys are not read
        for field, bound in (("user", t.num_users), ("account", t.num_accounts), ("qos", t.num_qos), ("user_acct", t.num_user_accts)):
            k = keys.slice(0, 64)
            getattr(k, field)[9] = bound
            k.skip[9] = 0
            with pytest.raises(EngineError) as e:
                eng.check_submissions(jobs, k)
            assert e.value.status == sp.ERR_INVALID_ARG, field
            k.skip[9] = 1
            eng.check_submissions(jobs, k)
        bad = sb.slice_jobs(jobs, 0, 64)
        bad.partition[3] = t.num_partitions
        keys.skip[3] = 0
        with pytest.raises(EngineError) as e:
            eng.check_submissions(bad, keys)
        assert e.value.status == sp.ERR_INVALID_ARG
        # the UINT32_MAX rule: the largest count of the tables + the sum of count over the call
        t.qos_submit[0] = 0xFFFFFFFF - 10
        eng.set_submit_limits(t)
        with pytest.raises(EngineError) as e:
            eng.check_submissions(jobs, keys)
        assert e.value.status == sp.ERR_UNSUPPORTED
        with pytest.raises(sp.Refused):
            sp.run(t, jobs, keys)
        few = keys.slice(0, 5)
        few.count[:] = 2
        few.skip[:] = 0
        _same("just inside the rule", eng.check_submissions(sb.slice_jobs(jobs, 0, 5), few), eng.submit_usage(), sp.run(t, sb.slice_jobs(jobs, 0, 5), few))
        t.acct_qos["jobs_count"][0] = 0xFFFFFFFF
        with pytest.raises(EngineError) as e:
            eng.set_submit_limits(t)
        assert e.value.status == sp.ERR_INVALID_ARG
        with pytest.raises(EngineError) as e:      # a failed set leaves no tables
            eng.check_submissions(jobs, keys)
        assert e.value.status == sp.ERR_STATE
        assert good[2] >= 0
    finally:
        eng.close()
