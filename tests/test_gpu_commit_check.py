"""The commit loop's checks behind a cycle (include/crane_gpu_commit/commit_check.h, csrc/commit_kernels.inc) on the GPU against
tests/commit_pyref.py, the restatement of JobScheduler.cpp:1464-1555, fed with the ENGINE's own downloaded placements: code and counts
for equality (all integers, no tolerance).  The hand-made cycle, the seeds of the generator (whose coverage condition is asserted on the
oracle's placements in tests/test_commit_pyref.py; here the engine's placements must equal them), the seams of the check kernel read from
cns_commit_shape, empty inputs, a cycle with preemption, the errors, independence of the other calls, and the chain the call exists
for: codes -> skip -> cns_apply_run_limits against the sequential loop of :1492-1573."""
import functools

import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd import limits as lm
from cranesched_amd.engine import EngineError
from tests import commit_case as cc
from tests import commit_pyref as ref
from tests import kat
from tests.test_reservations import _resv

pytestmark = pytest.mark.gpu
NOW, PAST, NONE = cc.NOW, cc.PAST, abi.RESV_NONE
FAR = NOW + 10 ** 6


def _want(pl, ev, cj):
    return ref.check(pl.start_sec, pl.reason, pl.place_offsets, pl.node_idx, ev, cj)


def _same(what, got, want):
    code, counts = got
    wcode, wcounts = want
    bad = np.flatnonzero(code != wcode)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(wcode)} jobs differ, first job {int(bad[0])}: got "
                           f"{abi.COMMIT_STR.get(int(code[bad[0]]), int(code[bad[0]]))}, want {abi.COMMIT_STR[int(wcode[bad[0]])]}")
    assert counts.tolist() == wcounts.tolist(), f"{what}: counts {counts.tolist()}, want {wcounts.tolist()}"


def _cycle(engine_default, cl, jobs, now=NOW, rv=None):
    eng = engine_default(device=0)
    try:
        eng.set_nodes(cl)
        if rv is not None:
            eng.set_reservations(rv)
        return eng, eng.node_select(now, jobs)
    except Exception:
        eng.close()
        raise


def _records(pl, j):
    return [int(n) for n in pl.node_idx[int(pl.place_offsets[j]):int(pl.place_offsets[j + 1])]]


# ---- 1. the hand-made cycle ------------------------------------------------------------------------------------------------------------
def test_hand_cycle(engine_default):
    cl, rv, jobs, now, ev, cj, sure = cc.hand()
    eng, pl = _cycle(engine_default, cl, jobs, now, rv)
    try:
        want = _want(pl, ev, cj)
        for j, c in sure:
            assert int(want[0][j]) == c, f"the restatement on the engine's placements, job {j}: {abi.COMMIT_STR[int(want[0][j])]}"
        _same("hand cycle", eng.commit_check(ev, cj), want)
        _same("hand cycle (again)", eng.commit_check(ev, cj), want)
    finally:
        eng.close()


# ---- 2. the generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cc.SEEDS)
def test_generated(engine_default, seed):
    cl, rv, jobs, now, ora, ev, cj, code, counts = cc.generated(seed)
    eng, pl = _cycle(engine_default, cl, jobs, now, rv)
    try:
        assert pl.diff(ora) is None, "the engine's placements are the oracle's (the coverage condition was asserted on those)"
        _same(f"seed {seed}", eng.commit_check(ev, cj), (code, counts))
    finally:
        eng.close()


# ---- 3. the seams of the check kernel --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shape():
    import ctypes as C
    from cranesched_amd import engine
    a, b = C.c_uint32(0), C.c_uint32(0)
    assert engine.lib().cns_commit_shape(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


SEAM_N = 140


def _seam_cluster(resv: bool):
    """140 nodes of 64 cores / 256 GiB in one partition, empty; `resv`: one active reservation takes every node whole."""
    cl = kat.cluster([64] * SEAM_N, mem_gib=[256] * SEAM_N)
    rv = _resv([(NOW - 10, FAR, [(n, 64, 256, 2 ** 64 - 1) for n in range(SEAM_N)])]) if resv else None
    return cl, rv


def _seam_jobs(widths, resv: bool):
    rows = [dict(L=100, k=k, **({"rsv": 0} if resv else {})) for k in widths]
    return cc.make_jobs(rows)


def _offend(node, resv: bool):
    """The call in which exactly `node` offends: a node event at InfinitePast, or the reservation's list without it."""
    if resv:
        return abi.CommitEvents(affected_resv=[(0, 1, FAR, [n for n in range(SEAM_N) if n != node][::-1])])
    return abi.CommitEvents(node_events=[(PAST, [node])])


def _seam_calls(eng, pl, jobs, targets, resv):
    cj = abi.CommitJobs(time_limit_sec=jobs.time_limit_sec, reservation=jobs.reservation)
    hit = abi.COMMIT_RESV_CHANGED if resv else abi.COMMIT_RESOURCE_CHANGED
    assert (pl.reason[:jobs.num_jobs] == 0).all(), "every job of a seam case starts"
    for j, pos in targets:
        recs = _records(pl, j)
        if pos >= len(recs):
            continue
        ev = _offend(recs[pos], resv)
        want = _want(pl, ev, cj)
        assert int(want[0][j]) == hit
        _same(f"job {j} ({len(recs)} records), record {pos} offends", eng.commit_check(ev, cj), want)
    none = abi.CommitEvents(affected_resv=[(0, 1, FAR, list(range(SEAM_N)))]) if resv else abi.CommitEvents(node_events=[(PAST, [])])
    want = _want(pl, none, cj)
    assert (want[0] == abi.COMMIT_OK).all()
    _same("nobody offends", eng.commit_check(none, cj), want)


@pytest.mark.parametrize("resv", [False, True], ids=["node_events", "reservation_list"])
def test_node_count_seams(engine_default, resv):
    """node_num 1, lane_max_nodes - 1, lane_max_nodes, lane_max_nodes + 1, 63, 64, 65 and 129; the one offending node is the job's first,
    last and 65th record in turn."""
    _, lane_max = _shape()
    widths = [1, lane_max - 1, lane_max, lane_max + 1, 63, 64, 65, 129]
    cl, rv = _seam_cluster(resv)
    jobs = _seam_jobs(widths, resv)
    eng, pl = _cycle(engine_default, cl, jobs, NOW, rv)
    try:
        targets = [(j, pos) for j, k in enumerate(widths) for pos in sorted({0, k - 1, 64})]
        _seam_calls(eng, pl, jobs, targets, resv)
    finally:
        eng.close()


@pytest.mark.parametrize("resv", [False, True], ids=["node_events", "reservation_list"])
@pytest.mark.parametrize("which", range(4))
def test_job_count_seams(engine_default, which, resv):
    """J = job_chunk - 1, job_chunk, job_chunk + 1 and 2 job_chunk + 1 one-node jobs, with a 129-node job as the last job of the first
    chunk, as the first job of the next, and as the last job of the queue."""
    chunk, _ = _shape()
    J = [chunk - 1, chunk, chunk + 1, 2 * chunk + 1][which]
    wide = sorted({j for j in (chunk - 1, chunk, J - 1) if j < J})
    widths = [129 if j in wide else 1 for j in range(J)]
    cl, rv = _seam_cluster(resv)
    jobs = _seam_jobs(widths, resv)
    eng, pl = _cycle(engine_default, cl, jobs, NOW, rv)
    try:
        _seam_calls(eng, pl, jobs, [(j, pos) for j in wide for pos in (0, 128)] + [(0, 0), (J - 2, 0)], resv)
    finally:
        eng.close()


# ---- 4. empty inputs -------------------------------------------------------------------------------------------------------------------
def test_empty_inputs(engine_default):
    cl, rv, jobs, now, ev, cj, _ = cc.hand()
    eng, pl = _cycle(engine_default, cl, jobs, now, rv)
    try:
        J = jobs.num_jobs
        bare = abi.CommitJobs(time_limit_sec=jobs.time_limit_sec, reservation=jobs.reservation)
        started = pl.reason[:J] == 0
        for e in (None, abi.CommitEvents()):
            code, counts = eng.commit_check(e, bare)
            assert np.array_equal(code, np.where(started, abi.COMMIT_OK, abi.COMMIT_NOT_STARTED)), "no events, no lists: every started job is OK"
            assert counts.tolist() == [int(started.sum()), 0, int(J - started.sum()), 0, 0, 0, 0, 0]
        every = abi.CommitEvents(node_events=[(PAST, list(range(cl.num_nodes)))])
        code, counts = eng.commit_check(every, bare)
        outside = started & (jobs.reservation == NONE)
        assert outside.any() and (started & ~outside).any()
        assert np.array_equal(code, np.where(outside, abi.COMMIT_RESOURCE_CHANGED, np.where(started, abi.COMMIT_OK, abi.COMMIT_NOT_STARTED)))
        _same("every node at InfinitePast", (code, counts), _want(pl, every, bare))
        # no started job: a queue into a partition that does not exist
        rows = [dict(part=5, L=100)] * 70
        nojobs = cc.make_jobs(rows)
        pl2 = eng.node_select(now, nojobs)
        assert (pl2.reason[:70] != 0).all()
        code, counts = eng.commit_check(every, abi.CommitJobs(time_limit_sec=nojobs.time_limit_sec))
        assert (code == abi.COMMIT_NOT_STARTED).all() and counts.tolist() == [0, 0, 70, 0, 0, 0, 0, 0]
        # an empty queue: counts only
        empty = cc.make_jobs([])
        eng.node_select(now, empty)
        code, counts = eng.commit_check(every, abi.CommitJobs(time_limit_sec=[]))
        assert len(code) == 0 and counts.tolist() == [0] * 8
    finally:
        eng.close()


# ---- 5. behind a cycle with preemption -------------------------------------------------------------------------------------------------
def test_behind_a_cycle_with_preemption(engine_default):
    from tests import kat_preempt
    name, c, j, r, pre, expect = kat_preempt.scenarios()[0]
    assert name == "preempt_running_job" and expect["preempted"] == {0: [(False, 0)]}
    eng = engine_default(device=0)
    try:
        eng.set_nodes(c)
        eng.set_running(r)
        pl, po = eng.node_select_preempt(kat_preempt.NOW, j, pre)
        assert po.lists() == [[(False, 0)]] and int(pl.reason[0]) == 0
        for alive, want in ((1, abi.COMMIT_WAITING_PREEMPTION), (0, abi.COMMIT_OK)):
            cj = abi.CommitJobs(time_limit_sec=j.time_limit_sec, preempt_offsets=po.offsets, preempted=po.preempted[:int(po.offsets[1])],
                                running_alive=[alive])
            got = eng.commit_check(None, cj)
            _same(f"victim alive = {alive}", got, _want(pl, None, cj))
            assert got[0].tolist() == [want]
        code, counts = eng.commit_check(None, abi.CommitJobs(time_limit_sec=j.time_limit_sec))          # preempt_offsets NULL
        assert code.tolist() == [abi.COMMIT_OK] and counts.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    finally:
        eng.close()


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(EngineError) as e:
        fn()
    assert len(str(e.value)) > 25, "a message comes with the status"
    return e.value.status


def test_errors(engine_default):
    cl, rv, jobs, now, ev, cj, _ = cc.hand()
    eng = engine_default(device=0)
    try:
        assert _refused(lambda: eng.commit_check(ev, cj)) == -5                               # before cns_set_nodes
        eng.set_nodes(cl)
        eng.set_reservations(rv)
        assert _refused(lambda: eng.commit_check(ev, cj)) == -5                               # before a cycle
        eng.upload_jobs(jobs)
        assert _refused(lambda: eng.commit_check(ev, cj)) == -5                               # jobs uploaded, nothing run
        pl = eng.node_select(now, jobs)
        want = _want(pl, ev, cj)
        J = jobs.num_jobs
        L, R = jobs.time_limit_sec, jobs.reservation

        def events(**kw):
            e = abi.CommitEvents(node_events=ev.node_events, affected_resv=ev.affected_resv)
            for k, v in kw.items():
                setattr(e, k, np.asarray(v, getattr(e, k).dtype))
            return e

        def lists(refs, alive):
            off = np.zeros(J + 1, np.uint64)
            off[1:] = len(refs)
            return abi.CommitJobs(time_limit_sec=L, reservation=R, preempt_offsets=off, preempted=refs, running_alive=alive)

        bad = [
            ("another num_jobs", lambda: eng.commit_check(ev, abi.CommitJobs(time_limit_sec=L[:-1], reservation=R[:-1]))),
            ("ev_offsets decrease", lambda: eng.commit_check(events(ev_offsets=[0, 4, 2, 12]), cj)),
            ("ar_offsets decrease", lambda: eng.commit_check(events(ar_offsets=[0, 1, 0, 2]), cj)),
            ("a node event beyond the node table", lambda: eng.commit_check(abi.CommitEvents(node_events=[(5, [1, cl.num_nodes])]), cj)),
            ("a reservation list beyond the node table", lambda: eng.commit_check(abi.CommitEvents(affected_resv=[(0, 1, FAR, [4, 99])]), cj)),
            ("no such reservation", lambda: eng.commit_check(abi.CommitEvents(affected_resv=[(3, 1, FAR, [4])]), cj)),
            ("a reservation named twice", lambda: eng.commit_check(abi.CommitEvents(affected_resv=[(1, 1, FAR, [6]), (1, 0, 0, [])]), cj)),
            ("a node twice in a reservation list", lambda: eng.commit_check(abi.CommitEvents(affected_resv=[(0, 1, FAR, [4, 5, 4])]), cj)),
            ("a running reference beyond the table", lambda: eng.commit_check(None, lists([2], [1, 0]))),
            ("running references without running_alive", lambda: eng.commit_check(None, lists([0], None))),
            ("preempt_offsets decrease", lambda: eng.commit_check(None, abi.CommitJobs(
                time_limit_sec=L, preempt_offsets=[0, 2, 1] + [2] * (J - 2), preempted=[0, 1], running_alive=[1, 0]))),
        ]
        for what, call in bad:
            assert _refused(call) == -1, what
            _same(f"after '{what}'", eng.commit_check(ev, cj), want)
        # a missing array, through the C structs (the Python classes always fill them)
        import ctypes as C
        code = np.zeros(J, np.uint8)
        c_ev, c_j = ev.to_c(), cj.to_c()
        c_j.time_limit_sec = None
        out = abi.CnsCommitOut(abi._ptr(code), None)
        assert eng._L.cns_commit_check(eng._h, C.byref(c_ev), C.byref(c_j), C.byref(out), None) == -1
        c_j = cj.to_c()
        assert eng._L.cns_commit_check(eng._h, C.byref(c_ev), C.byref(c_j), C.byref(abi.CnsCommitOut(None, None)), None) == -1
        c_ev.ev_nodes = None
        assert eng._L.cns_commit_check(eng._h, C.byref(c_ev), C.byref(c_j), C.byref(out), None) == -1
        assert eng._L.cns_commit_check(eng._h, C.byref(ev.to_c()), C.byref(c_j), C.byref(out), None) == 0      # counts may be NULL
        assert np.array_equal(code, want[0])
        # a node twice inside one node event is the reference's fold, not an error
        twice = abi.CommitEvents(node_events=[(NOW + 100, [0, 0, 1, 2, 3, 3])])
        _same("a node twice in a node event", eng.commit_check(twice, cj), _want(pl, twice, cj))
    finally:
        eng.close()


# ---- 7. independence -------------------------------------------------------------------------------------------------------------------
def _one_user_tables():
    return lm.LimitTables(num_users=1, num_user_accts=1, num_partitions=2, qos=np.array([lm.qos_limits(max_jobs_per_user=7)], lm.QOS_DT),
                          acct_parent=np.array([lm.LIM_NONE], np.uint32))


def test_the_other_calls_do_not_see_it(engine_default):
    """A download, a probe, a validity call and the run-limit admission give identical bytes with and without a commit_check in front."""
    from tests import probe_case as pc
    c, j, p, now, run, rv = pc.resv_scenario(0)
    J = j.num_jobs
    t = _one_user_tables()
    lj = lm.LimitJobs(user=[0] * J, user_acct=[0] * J, account=[0] * J, qos=[0] * J, partition=[0] * J, time_limit_sec=j.time_limit_sec)
    cj = abi.CommitJobs(time_limit_sec=j.time_limit_sec, reservation=j.reservation)
    ev = abi.CommitEvents(node_events=[(now + 50, list(range(0, c.num_nodes, 2)))], affected_resv=[(0, 1, now + 10, [])])
    plain, mixed = engine_default(device=0), engine_default(device=0)

    def run_all(eng, check):
        out = {}
        eng.set_nodes(c)
        eng.set_reservations(rv)
        eng.set_running(run)
        eng.set_run_limits(t)
        sel = eng.node_select(now, j)
        commit = []
        for step in ("download", "probe", "validate", "limits"):
            if check:
                commit.append(eng.commit_check(ev, cj))
            if step == "download":
                out[step] = eng.download()
            elif step == "probe":
                out[step] = eng.probe(p)
            elif step == "validate":
                out[step] = eng.validate_jobs(j)
            else:
                out[step] = eng.apply_run_limits(lj) + (eng.usage(),)
        if check:
            commit.append(eng.commit_check(ev, cj))
        return sel, out, commit

    try:
        sel0, a, _ = run_all(plain, False)
        sel1, b, commit = run_all(mixed, True)
        assert sel1.diff(sel0) is None
        assert b["download"].diff(a["download"]) is None and b["download"].diff(sel0) is None
        assert b["probe"].diff(a["probe"]) is None
        assert np.array_equal(b["validate"][0], a["validate"][0]) and np.array_equal(b["validate"][1], a["validate"][1])
        assert np.array_equal(b["limits"][0], a["limits"][0]) and b["limits"][1] == a["limits"][1] and b["limits"][2].same_as(a["limits"][2])
        want = _want(sel0, ev, cj)
        assert len(set(want[0].tolist())) >= 3
        for i, got in enumerate(commit):
            _same(f"commit_check number {i} between the other calls", got, want)
    finally:
        plain.close()
        mixed.close()


# ---- 8. the chain it exists for --------------------------------------------------------------------------------------------------------
def test_codes_as_skip_make_the_admission_exact(engine_default):
    """One user under max_jobs_per_user = 1.  Job 0 (L 101) loses its node at NOW+100: "Resource changed" (:1518), the loop continues
    before the admission, and job 1 is the one admitted.  Without the skip job 0 takes the user's only slot and job 1 is refused."""
    from oracle import pyoracle
    cl = kat.cluster([4, 4])
    jobs = kat.jobs([dict(L=101), dict(L=50), dict(L=50)])
    ev = abi.CommitEvents(node_events=[(NOW + 100, [0, 1])])
    cj = abi.CommitJobs(time_limit_sec=jobs.time_limit_sec)
    t = lm.LimitTables(num_users=1, num_user_accts=1, num_partitions=1, qos=np.array([lm.qos_limits(max_jobs_per_user=1)], lm.QOS_DT),
                       acct_parent=np.array([lm.LIM_NONE], np.uint32))

    def lim_jobs(skip):
        return lm.LimitJobs(user=[0] * 3, user_acct=[0] * 3, account=[0] * 3, qos=[0] * 3, partition=[0] * 3, time_limit_sec=jobs.time_limit_sec,
                            skip=skip)

    eng, pl = _cycle(engine_default, cl, jobs)
    try:
        assert (pl.reason[:3] == 0).all()
        # the sequential loop of :1492-1573: the restatement's codes are its `continue`s, the CPU port of the limits is its admission
        want_code, _ = _want(pl, ev, cj)
        assert want_code.tolist() == [abi.COMMIT_RESOURCE_CHANGED, abi.COMMIT_OK, abi.COMMIT_OK]
        want_reason, want_adm, want_usage = pyoracle.run_limits(cl.gres, t, lim_jobs(want_code != abi.COMMIT_OK), pl)
        code, _ = eng.commit_check(ev, cj)
        eng.set_run_limits(t)
        reason, adm = eng.apply_run_limits(lim_jobs(code != abi.COMMIT_OK))
        assert np.array_equal(reason, want_reason) and adm == want_adm == 1 and eng.usage().same_as(want_usage)
        assert int(reason[1]) == 0 and int(reason[0]) == 255 and int(reason[2]) not in (0, 255)
        eng.set_run_limits(t)
        blind, adm2 = eng.apply_run_limits(lim_jobs(None))
        assert not np.array_equal(blind, reason), "without the skip the dropped job is admitted and the usage it leaves refuses job 1"
        assert int(blind[0]) == 0 and int(blind[1]) not in (0, 255) and adm2 == 1
    finally:
        eng.close()
