"""The pending gate (include/crane_gpu_gate/pending_gate.h, csrc/gate_kernels.inc) on the GPU against tests/gate_pyref.py, the
restatement of JobScheduler.cpp:1353-1413: code, pending, ready_sec, dep_erased, counts and ev_stats for equality (all integers, no
tolerance).  The case list (tests/gate_case.py) is built from cns_gate_shape and puts a case on every seam of the kernels; then the
hand-derived table's own expectations, buffer reuse on one handle, a fresh handle, independence of a cycle, the errors."""
import ctypes as C
import functools

import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.engine import EngineError
from tests import gate_case as gc
from tests import gate_pyref as ref

pytestmark = pytest.mark.gpu
NOW = gc.NOW


@functools.lru_cache(maxsize=None)
def _shape():
    from cranesched_amd import engine
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert engine.lib().cns_gate_shape(C.byref(a), C.byref(b), C.byref(c)) == 0
    return a.value, b.value, c.value


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (now, jobs, events, packed jobs, packed events, (Result, dep_erased, jobs after)): the reference is computed once."""
    out = {}
    for name, now, jobs, events in gc.seam_cases(*_shape()):
        out[name] = (now, jobs, events, gc.pack(jobs), gc.pack_events(events), gc.expected(now, jobs, events))
    return out


# (the names are fixed by the shipped shape; test_the_case_list_follows_the_shape holds the two together)
CASE_NAMES = [c[0] for c in gc.seam_cases(256, 8, 256)]


def _same(what, got, want):
    res, erased, _ = want
    code, pending, ready, er, counts, stats = got
    bad = np.flatnonzero(code != res.code)
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(res.code)} codes differ, first row {int(bad[0])}: got "
                           f"{abi.GATE_STR.get(int(code[bad[0]]), int(code[bad[0]]))}, want {abi.GATE_STR[int(res.code[bad[0]])]}")
    assert np.array_equal(ready, res.ready_sec), f"{what}: ready_sec differs at rows {np.flatnonzero(ready != res.ready_sec)[:5].tolist()}"
    assert np.array_equal(er, erased), f"{what}: dep_erased differs at entries {np.flatnonzero(er != erased)[:5].tolist()}"
    assert len(pending) == len(res.pending) and np.array_equal(pending, res.pending), f"{what}: pending differs"
    assert counts.tolist() == res.counts.tolist(), f"{what}: counts {counts.tolist()}, want {res.counts.tolist()}"
    assert stats.tolist() == res.ev_stats.tolist(), f"{what}: ev_stats {stats.tolist()}, want {res.ev_stats.tolist()}"


@pytest.fixture(scope="module")
def eng(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from cranesched_amd.engine import GpuNodeSelector
    e = GpuNodeSelector(device=0)   # a fresh handle: no snapshot, no cycle
    yield e
    e.close()


def test_the_case_list_follows_the_shape(built):
    chunk, lane_max, span = _shape()
    assert (chunk, lane_max, span) == (256, 8, 256) and list(_cases()) == CASE_NAMES
    assert {f"J{chunk + 1}", f"scan_J{span * 64 - 1}", f"scan_J{span * 64 + 1}", "two_long_lists_in_a_wave", "repeat70_asc_and", "E65"} <= set(CASE_NAMES)


# ---- 1. every seam -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_seam_case(eng, name):
    now, jobs, events, pj, pe, want = _cases()[name]
    _same(name, eng.gate_pending(now, pj, pe if events else None), want)


def test_the_table_rows_on_the_device(eng):
    """The hand-derived expectations themselves, not only the restatement's: every row of the table as a queue of one."""
    for name, now, job, events, code, ready, left in gc.table():
        got = eng.gate_pending(now, gc.pack([job]), gc.pack_events(events))
        assert (int(got[0][0]), int(got[2][0]), len(got[3]) - int(got[3].sum())) == (code, ready, left), name
        assert got[1].tolist() == ([0] if code <= abi.GATE_OK_ARRAY_PARENT else []), name


def test_every_array_given_or_left_out(eng):
    """The optional arrays as NULL and as arrays of the neutral value give the same answer; an empty event list is no events."""
    jobs, _ = gc.pattern(300, range(0, 300, 3))
    for j in jobs:
        j.held = False
    want = gc.expected(NOW, jobs, [])
    for opt in (True, False):
        _same(f"optional arrays left out: {opt}", eng.gate_pending(NOW, gc.pack(jobs, optional=opt), None), want)
    _same("an empty event list", eng.gate_pending(NOW, gc.pack(jobs), gc.pack_events([])), want)
    assert gc.pack(jobs).held is None and gc.pack(jobs).dep_offsets is None and gc.pack(jobs).array_parent is None


# ---- 2. one handle, again and again ------------------------------------------------------------------------------------------------------
def test_buffer_reuse_across_sizes(eng):
    """Large, small, large on one handle: a smaller call inside grown buffers, and nothing of the call before shows."""
    names = ["random_3000x5000", "J1", "list_lengths", "pattern_none_ok", "random_3000x5000", "E0"]
    for n in names:
        now, jobs, events, pj, pe, want = _cases()[n]
        _same(f"{n} in a sequence", eng.gate_pending(now, pj, pe if events else None), want)


def test_empty_queue(eng):
    empty = abi.GateJobs(job_id=[])
    code, pending, ready, erased, counts, stats = eng.gate_pending(NOW, empty, gc.pack_events([(1, 2, 3), (4, 5, 6)]))
    assert len(code) == 0 and len(pending) == 0 and counts.tolist() == [0] * 16 and stats.tolist() == [0, 2, 0]
    code, pending, ready, erased, counts, stats = eng.gate_pending(NOW, empty, None)
    assert len(code) == 0 and stats.tolist() == [0, 0, 0]


def test_the_tail_of_pending_is_not_touched(eng):
    jobs, _ = gc.pattern(100, (5, 50))
    pj = gc.pack(jobs)
    code, pending = np.zeros(100, np.uint8), np.full(100, 0xABCD, np.uint32)
    n = np.zeros(1, np.uint64)
    out = abi.CnsGateOut(abi._ptr(code), abi._ptr(pending), abi._ptr(n), None, None, None, None)   # every optional result NULL
    assert eng._L.cns_gate_pending(eng._h, C.c_int64(NOW), C.byref(pj.to_c()), None, C.byref(out), None) == 0
    assert int(n[0]) == 2 and pending[:2].tolist() == [5, 50] and (pending[2:] == 0xABCD).all()


# ---- 3. beside a cycle -------------------------------------------------------------------------------------------------------------------
def test_a_cycle_does_not_see_it(engine_default):
    """cns_select, the gate, cns_download: the download is the selection's; and the gate's answer behind a cycle is the fresh handle's."""
    from cranesched_amd import synth
    cluster, jobs, now = synth.make_config("C1")
    now_g, qj, qe, pj, pe, want = _cases()["two_long_lists_in_a_wave"]
    e = engine_default(device=0)
    try:
        _same("before any snapshot", e.gate_pending(now_g, pj, pe), want)
        e.set_nodes(cluster)
        sel = e.node_select(now, jobs)
        _same("behind a cycle", e.gate_pending(now_g, pj, pe), want)
        assert e.download().diff(sel) is None
        assert e.node_select(now, jobs).diff(sel) is None
    finally:
        e.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------
def _refused(fn):
    with pytest.raises(EngineError) as e:
        fn()
    assert "cns_gate_pending" in str(e.value) and len(str(e.value)) > 30, "a message comes with the status"
    return e.value.status


def test_errors(eng):
    now, jobs, events, pj, pe, want = _cases()["list_lengths"]

    def changed(**kw):
        g = gc.pack(jobs)
        for k, v in kw.items():
            setattr(g, k, None if v is None else np.asarray(v, getattr(g, k).dtype))
        return g

    ids, off, dj = pj.job_id.copy(), pj.dep_offsets.copy(), pj.dep_job.copy()
    dup = ids.copy(); dup[5] = dup[4]
    desc = ids.copy(); desc[[7, 8]] = desc[[8, 7]]
    off1 = off.copy(); off1[0] = 1
    offd = off.copy(); offd[3] = offd[4] + 1
    b = int(off[3])                                # row 3 has lane_max + 1 entries
    same = dj.copy(); same[b + 1] = same[b]
    swap = dj.copy(); swap[[b + 1, b + 2]] = swap[[b + 2, b + 1]]
    J = len(ids)
    ap = dict(array_parent=np.ones(J), ap_flags=np.full(J, 31), ap_deadline_sec=np.zeros(J), ap_running=np.zeros(J), ap_run_limit=np.ones(J))

    def with_ap(**kw):
        g = gc.pack(jobs)
        for k, v in {**ap, **kw}.items():
            setattr(g, k, None if v is None else np.ascontiguousarray(v, dtype=dict(abi.GateJobs._DTYPES)[k]))
        return g

    flags = np.full(J, 31); flags[J - 1] = 32
    bad = [
        ("job_id repeats", lambda: eng.gate_pending(now, changed(job_id=dup), pe)),
        ("job_id descends", lambda: eng.gate_pending(now, changed(job_id=desc), pe)),
        ("dep_offsets[0] != 0", lambda: eng.gate_pending(now, changed(dep_offsets=off1), pe)),
        ("dep_offsets decrease", lambda: eng.gate_pending(now, changed(dep_offsets=offd), pe)),
        ("a dependee twice in a list", lambda: eng.gate_pending(now, changed(dep_job=same), pe)),
        ("a list that descends", lambda: eng.gate_pending(now, changed(dep_job=swap), pe)),
        ("entries without dep_job", lambda: eng.gate_pending(now, changed(dep_job=None), pe)),
        ("entries without dep_delay_sec", lambda: eng.gate_pending(now, changed(dep_delay_sec=None), pe)),
        ("dep_is_or without dep_ready_sec", lambda: eng.gate_pending(now, changed(dep_ready_sec=None), pe)),
        ("entries without dep_is_or", lambda: eng.gate_pending(now, changed(dep_is_or=None, dep_ready_sec=None), pe)),
        ("array_parent without ap_flags", lambda: eng.gate_pending(now, with_ap(ap_flags=None), pe)),
        ("array_parent without ap_run_limit", lambda: eng.gate_pending(now, with_ap(ap_run_limit=None), pe)),
        ("an ap_flags bit outside the mask", lambda: eng.gate_pending(now, with_ap(ap_flags=flags), pe)),
    ]
    for what, call in bad:
        assert _refused(call) == -1, what
        _same(f"after '{what}'", eng.gate_pending(now, pj, pe), want)
    # missing arrays through the C structs
    code, pending, n = np.zeros(J, np.uint8), np.zeros(J, np.uint32), np.zeros(1, np.uint64)
    cj, ce = pj.to_c(), pe.to_c()
    full = abi.CnsGateOut(abi._ptr(code), abi._ptr(pending), abi._ptr(n), None, None, None, None)
    for out in (abi.CnsGateOut(None, abi._ptr(pending), abi._ptr(n)), abi.CnsGateOut(abi._ptr(code), None, abi._ptr(n)), abi.CnsGateOut(abi._ptr(code), abi._ptr(pending), None)):
        assert eng._L.cns_gate_pending(eng._h, C.c_int64(now), C.byref(cj), C.byref(ce), C.byref(out), None) == -1
    ce.event_sec = None
    assert eng._L.cns_gate_pending(eng._h, C.c_int64(now), C.byref(cj), C.byref(ce), C.byref(full), None) == -1
    cj.job_id = None
    assert eng._L.cns_gate_pending(eng._h, C.c_int64(now), C.byref(cj), None, C.byref(full), None) == -1
    assert eng._L.cns_gate_pending(eng._h, C.c_int64(now), None, None, C.byref(full), None) == -1
    # the sizes the 32-bit indices do not hold: refused before any array is read
    big = pj.to_c(); big.num_jobs = (1 << 32) - 511
    assert eng._L.cns_gate_pending(eng._h, C.c_int64(now), C.byref(big), None, C.byref(full), None) == -4
    ce = pe.to_c(); ce.num_events = (1 << 32) - 255
    assert eng._L.cns_gate_pending(eng._h, C.c_int64(now), C.byref(pj.to_c()), C.byref(ce), C.byref(full), None) == -4
    _same("after the refusals", eng.gate_pending(now, pj, pe), want)
