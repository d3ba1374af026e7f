"""Reservation what-ifs (include/crane_gpu_resv/resv_probe.h, csrc/resvq_kernels.inc) on the GPU against tests/resvq_pyref.py, the
restatement of JobScheduler::CreateResv_'s node walk: every output array, for equality.  Random clusters (tests/resvq_case.py), lists
across the wave / workgroup / chunk edges of the pick kernel, both modes in one call, more queries than the pick kernel has
workgroups; the calls are read-only and repeatable, leave a cycle and a probe as they were, and refuse what the header says.

The expected answers are computed once per scenario and shared."""
import functools

import numpy as np
import pytest

from cranesched_amd import abi
from cranesched_amd.engine import EngineError
from tests import resvq_case as rc
from tests import resvq_pyref as ref

pytestmark = pytest.mark.gpu

# name -> (seed, nodes or None: drawn from 1..300, queries)
SCENARIOS = {"one": (0, None, 1), "many": (1, 300, 257), "mid": (2, None, 24), "tiny": (3, 1, 16), "small": (4, 7, 40)}


@functools.lru_cache(maxsize=None)
def scenario(name):
    seed, N, Q = SCENARIOS[name]
    cluster, running, resv, times = rc.random_cluster(seed, N)
    state = ref.NodeState(cluster.num_nodes, running, resv)
    lengths = rc.LIST_LENGTHS if name != "one" else (513,)
    queries = rc.random_queries(seed, cluster.num_nodes, state, times, Q, lengths)
    return cluster, running, resv, queries, state


@functools.lru_cache(maxsize=None)
def expected_of(name):
    cluster, running, resv, queries, state = scenario(name)
    return ref.answer(state, rc.NOW, queries)


def _engine(engine_default, cluster, running, resv):
    eng = engine_default(device=0)
    eng.set_nodes(cluster)
    eng.set_resv_query_state(running, resv)
    return eng


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_parity(engine_default, name):
    cluster, running, resv, queries, _ = scenario(name)
    eng = _engine(engine_default, cluster, running, resv)
    try:
        got = eng.query_reservations(rc.NOW, queries)
        rc.same(name, got, expected_of(name))
        again = eng.query_reservations(rc.NOW, queries)            # the same call twice: the same arrays
        rc.same(name + " (again)", again, got)
    finally:
        eng.close()


def test_coverage_of_the_scenarios(built):
    """Asserted on the RESTATEMENT's answers: all three statuses, all four codes, both modes with every status they can have, an
    earliest start later than the asked one, every list length and k on both sides of num_free, equal event times."""
    status, codes, lengths, later, mode_status = set(), set(), set(), 0, set()
    for name in SCENARIOS:
        cluster, running, resv, q, state = scenario(name)
        exp = expected_of(name)
        status |= set(exp["status"].tolist())
        codes |= set(exp["code"].tolist())
        lengths |= set(np.diff(q.cand_offsets.astype(np.int64)).tolist())
        mode_status |= set(zip(q.find_earliest.tolist(), exp["status"].tolist()))
        later += int(((exp["status"] == ref.OK) & (exp["start_sec"] > q.start_sec)).sum())
        ends = [e for n in range(state.num_nodes) for e in state.job_ends[n]] + [ed for n in range(state.num_nodes) for _, ed in state.resv[n]]
        if len(ends) > 20:
            assert len(set(ends)) <= 10, f"{name}: the ends are meant to collide"
    assert status == {ref.OK, ref.NOT_ENOUGH, ref.IN_THE_PAST}
    assert codes == {ref.FREE, ref.RUNNING, ref.RESERVED, ref.NOT_FOUND}
    assert lengths >= set(rc.LIST_LENGTHS)
    assert mode_status >= {(m, s) for m in (0, 1) for s in (ref.OK, ref.NOT_ENOUGH, ref.IN_THE_PAST)}
    assert later >= 5, "earliest-start queries that have to wait"


def test_permuting_the_queries_permutes_the_answers(engine_default):
    cluster, running, resv, queries, _ = scenario("mid")
    exp = expected_of("mid")
    order = np.random.default_rng(5).permutation(queries.num_queries)
    eng = _engine(engine_default, cluster, running, resv)
    try:
        got = eng.query_reservations(rc.NOW, queries.take(order))
    finally:
        eng.close()
    for f in ("status", "start_sec", "num_free"):
        assert np.array_equal(got[f], exp[f][order]), f
    for off, arr, eoff in (("chosen_offsets", "chosen_nodes", exp["chosen_offsets"]), (None, "code", queries.cand_offsets)):
        goff = got[off] if off else queries.take(order).cand_offsets
        for i, src in enumerate(order):
            assert np.array_equal(got[arr][int(goff[i]):int(goff[i + 1])], exp[arr][int(eoff[src]):int(eoff[src + 1])]), (arr, i)


def test_a_cycle_and_a_probe_do_not_notice(engine_default):
    """cns_select and cns_probe before and after cns_resvq_set_state / cns_resvq_run: identical to a handle that never saw the new calls."""
    from tests import probe_case as pc
    c, j, p, now, run, rv = pc.resv_scenario(0)
    _, qrun, qrv, queries, _ = scenario("small")        # 7 nodes: valid on every cluster of the cycle's scenario

    def cycle(eng):
        eng.set_nodes(c)
        eng.set_reservations(rv)
        eng.set_running(run)
        return eng.node_select(now, j), eng.probe(p)

    plain = engine_default(device=0)
    mixed = engine_default(device=0)
    try:
        want_sel, want_probe = cycle(plain)
        sel0, probe0 = cycle(mixed)
        assert sel0.diff(want_sel) is None and probe0.diff(want_probe) is None
        assert c.num_nodes >= 7
        mixed.set_resv_query_state(qrun, qrv)
        first = mixed.query_reservations(rc.NOW, queries)
        assert mixed.probe(p).diff(want_probe) is None, "a probe behind the reservation queries"
        assert mixed.download().diff(want_sel) is None, "the cycle's results behind the reservation queries"
        assert np.array_equal(mixed.costs().view(np.uint64), plain.costs().view(np.uint64))
        sel1 = mixed.node_select(now, j)
        assert sel1.diff(want_sel) is None and mixed.probe(p).diff(want_probe) is None
        rc.same("behind another cycle", mixed.query_reservations(rc.NOW, queries), first)   # ... and the cycle left the tables alone
    finally:
        plain.close()
        mixed.close()


def _status(fn):
    with pytest.raises(EngineError) as e:
        fn()
    return e.value.status


def _q(start=rc.NOW, dur=600, k=1, cand=(0, 1, 2), mode=0):
    return abi.ResvQueries([start], [dur], [k], [0, len(cand)], np.array(cand, np.uint32), [mode])


def test_state_machine_and_arguments(engine_default, monkeypatch):
    cluster, running, resv, queries, state = scenario("small")
    eng = engine_default(device=0)
    try:
        assert _status(lambda: eng.set_resv_query_state(running, resv)) == -5       # before cns_set_nodes
        assert _status(lambda: eng.query_reservations(rc.NOW, _q())) == -5
        eng.set_nodes(cluster)
        assert _status(lambda: eng.query_reservations(rc.NOW, _q())) == -5          # before cns_resvq_set_state
        eng.set_resv_query_state(None, None)                                        # no table at all: every found node is free
        got = eng.query_reservations(rc.NOW, _q(cand=(3, 99, 1), k=0))
        assert got["status"].tolist() == [ref.NOT_ENOUGH] and got["code"].tolist() == [0, 3, 0] and got["num_free"].tolist() == [2]
        eng.set_resv_query_state(running, resv)
        ok = eng.query_reservations(rc.NOW, queries)
        eng.set_nodes(cluster)                                                      # a new snapshot invalidates the tables
        assert _status(lambda: eng.query_reservations(rc.NOW, _q())) == -5
        eng.set_resv_query_state(running, resv)
        rc.same("after a new set_state", eng.query_reservations(rc.NOW, queries), ok)
        # arguments
        assert _status(lambda: eng.query_reservations(rc.NOW, _q(cand=(0, 1, 0)))) == -1      # a node twice
        assert _status(lambda: eng.query_reservations(rc.NOW, _q(cand=(0, 77, 77)))) == -1    # ... also one that does not exist
        assert _status(lambda: eng.query_reservations(rc.NOW, _q(dur=0))) == -1
        assert _status(lambda: eng.query_reservations(rc.NOW, _q(dur=-5))) == -1
        assert _status(lambda: eng.query_reservations(rc.NOW, _q(start=ref.INT64_MAX - 10, dur=11))) == -1   # overflow
        edge = _q(start=ref.INT64_MAX - 10, dur=10, mode=1, k=0)                                             # ... the last sum that fits
        rc.same("the last start", eng.query_reservations(rc.NOW, edge), ref.answer(state, rc.NOW, edge))
        q = _q(k=2)
        assert _status(lambda: eng.query_reservations(rc.NOW, q, abi.ResvAnswers(q, code_capacity=2))) == -1
        assert _status(lambda: eng.query_reservations(rc.NOW, q, abi.ResvAnswers(q, chosen_capacity=1))) == -1
        # Q = 0: CNS_OK and nothing written
        none = abi.ResvQueries([], [], [], [0], [], [])
        out = abi.ResvAnswers(none)
        for a in (out.status, out.start_sec, out.num_free, out.code, out.chosen_nodes, out.chosen_offsets):
            a[:] = 77
        eng.query_reservations(rc.NOW, none, out)
        assert all((a == 77).all() for a in (out.status, out.start_sec, out.num_free, out.code, out.chosen_nodes, out.chosen_offsets))
        # the interval cap, lowered through the environment: an earliest-start query over 3 found nodes costs at least 3 intervals
        monkeypatch.setenv("CNS_RESVQ_MAX_INTERVALS", "2")
        assert _status(lambda: eng.query_reservations(rc.NOW, _q(mode=1))) == -4
        eng.query_reservations(rc.NOW, _q(mode=0))                                  # a given start costs none
        monkeypatch.delenv("CNS_RESVQ_MAX_INTERVALS")
        rc.same("after the refusals", eng.query_reservations(rc.NOW, queries), ok)
    finally:
        eng.close()
