"""The step scheduler's checkers on the edge families of tests/steps_edge.py, without a GPU: mask algebra == literal-container algebra,
the oracle == the independent Python restatement (tests/steps_pyref.py), and — where oracle/_ref is built — == the reference's own
compiled JobInCtld::SchedulePendingSteps.  Then every family proves FROM THE ORACLE'S RESULT that it reaches the edge it is for (queues of
63 / 64 entries with ties, evictions from a full queue, tasks that carry GRES, a refusal for GRES alone, both sides of a block boundary),
so that an edit to a generator cannot step off the edge unnoticed.  tests/test_gpu_steps_edge.py runs the same cases on the engine."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import steps_edge as se
from tests.test_steps import _compare_steps

_CACHE = {}


def oracle_case(name):
    """(layout, jobs, steps, the oracle's result) of a case of steps_edge.CASES: built once, shared by the tests, never written to"""
    if name not in _CACHE:
        lay, jobs, steps = se.CASES[name]()
        _CACHE[name] = (lay, jobs, steps, pyoracle.schedule_steps(lay, jobs, steps))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(se.CASES))
def test_checkers_agree(name):
    lay, jobs, steps, a = oracle_case(name)
    b = pyoracle.schedule_steps(lay, jobs, steps, pyoracle.LITERAL)
    assert a.diff(b) is None, a.diff(b)
    _compare_steps(lay, jobs, steps, a)
    if pyoracle.ref_available():
        r = pyoracle.schedule_steps(lay, jobs, steps, backend="ref")
        assert a.diff(r) is None, a.diff(r)


def _scheduled_steps(jobs, steps, res):
    """(job, step, the step's node records as a slice) of every scheduled step"""
    for j in range(jobs.num_jobs):
        for s in range(int(jobs.step_offsets[j]), int(jobs.step_offsets[j + 1])):
            if res.scheduled[s]:
                yield j, s, slice(int(res.place_offsets[s]), int(res.place_offsets[s + 1]))


def test_deep_heap_reaches_the_heap_capacity():
    seen, tie = set(), False
    for seed in se.DEEP_HEAP_SEEDS:
        lay, jobs, steps, res = oracle_case(f"deep_heap-{seed}")
        for j, s, pl in _scheduled_steps(jobs, steps, res):
            k = int(steps.node_num[s])
            seen.add(k)
            nt = res.node_ntasks[pl]
            # nodes that got two or more tasks got all they hold (the spare tasks had not run out): equal counts there were equal in the queue
            tie |= k >= 32 and len(nt[nt >= 2]) > len(set(nt[nt >= 2].tolist()))
    assert {32, 33, 63, 64} <= seen, sorted(seen)
    assert tie


def test_eviction_ladder_evicts_and_stops_early():
    lay, jobs, steps, res = oracle_case("eviction_ladder")
    assert list(res.scheduled[:4]) == [1, 1, 1, 1]
    job0 = jobs.node_idx[:se.LADDER_NODES]
    for s, k in ((0, 64), (1, 33), (2, 32)):
        assert steps.node_num[s] == k
        got = set(res.node_idx[int(res.place_offsets[s]):int(res.place_offsets[s + 1])].tolist())
        assert len(got) == k and got != set(job0[:k].tolist()), f"step {s} kept the first {k} nodes: nothing was evicted"
    # step 0: the 16 one-core nodes are the ones that left the queue, and the walk reached the job's last node
    assert set(res.node_idx[:64].tolist()) == {int(n) for i, n in enumerate(job0) if i % 5 != 0}
    assert int(job0[-1]) in set(res.node_idx[:64].tolist())
    early = jobs.node_idx[se.LADDER_NODES:]
    s = 3
    got = res.node_idx[int(res.place_offsets[s]):int(res.place_offsets[s + 1])]
    assert sorted(got.tolist()) == early[:32].tolist() and list(res.node_ntasks[int(res.place_offsets[s]):int(res.place_offsets[s + 1])]) == [2] * 32


@pytest.mark.parametrize("name", [n for n in se.CASES if n.startswith("task_gres")])
def test_task_gres_reaches_the_task_loop(name):
    lay, jobs, steps, res = oracle_case(name)
    S = steps.num_steps
    assert steps.task_gres_total.any(axis=1).all(), "every step's task request carries GRES"
    assert res.task_gres.any(), "no task record holds a GRES slot"
    two = False
    for j, s, pl in _scheduled_steps(jobs, steps, res):
        t = slice(int(res.task_offsets[s]), int(res.task_offsets[s + 1]))
        assert (res.task_gres[t] != 0).all()
        two |= bool((res.node_ntasks[pl] >= 2).any())
    assert two, "no node was handed two GRES-carrying tasks"
    # a step refused for GRES alone: the first pending step of some job is scheduled once its tasks ask for no GRES
    for j in range(jobs.num_jobs):
        pend = [s for s in range(int(jobs.step_offsets[j]), int(jobs.step_offsets[j + 1])) if not res.scheduled[s]]
        if pend and pyoracle.schedule_steps(lay, jobs, se.without_task_gres(steps, pend[0])).scheduled[pend[0]]:
            break
    else:
        pytest.fail("no step is refused for its task GRES alone")
    assert 0 < res.scheduled[:S].sum() < S


def test_exact_fit_expectations():
    lay, jobs, steps, exp = se.exact_fit()
    res = oracle_case("exact_fit")[3]
    N = jobs.num_nodes
    assert list(res.avail_cpu_raw[:N]) == exp["avail_cpu"] and list(res.avail_mem[:N]) == exp["avail_mem"] and list(res.avail_core_lo[:N]) == exp["avail_core_lo"]
    for j in range(jobs.num_jobs):
        ss = range(int(jobs.step_offsets[j]), int(jobs.step_offsets[j + 1]))
        assert [int(res.scheduled[s]) for s in ss] == exp["scheduled"][j], f"job {j}"
        pl = np.concatenate([np.arange(res.place_offsets[s], res.place_offsets[s + 1], dtype=np.int64) for s in ss if res.scheduled[s]] + [np.zeros(0, np.int64)])
        tk = np.concatenate([np.arange(res.task_offsets[s], res.task_offsets[s + 1], dtype=np.int64) for s in ss if res.scheduled[s]] + [np.zeros(0, np.int64)])
        assert list(res.node_idx[pl]) == exp["node_idx"][j] and list(res.node_ntasks[pl]) == exp["node_ntasks"][j], f"job {j}"
        assert list(res.task_node[tk]) == exp["task_node"][j] and list(res.task_core_lo[tk]) == exp["task_core_lo"][j], f"job {j}"
        for s in ss:   # what a pending step owns stays at its fill values
            if not res.scheduled[s]:
                assert (res.node_idx[int(res.place_offsets[s]):int(res.place_offsets[s + 1])] == 0xFFFFFFFF).all()
                assert (res.task_node[int(res.task_offsets[s]):int(res.task_offsets[s + 1])] == 0xFFFFFFFF).all()
    x = exp["straddle"]
    s = steps.num_steps - 1
    t = slice(int(res.task_offsets[s]), int(res.task_offsets[s + 1]))
    assert list(res.task_core_hi[t]) == x["task_core_hi"] and list(res.task_core_w2[t]) == x["task_core_w2"] and list(res.task_core_w3[t]) == x["task_core_w3"]
    p = int(res.place_offsets[s])
    node = int(res.node_core_lo[p]) | int(res.node_core_hi[p]) << 64 | int(res.node_core_w2[p]) << 128 | int(res.node_core_w3[p]) << 192
    assert node == x["node_core"]


@pytest.mark.parametrize("J", se.LAUNCH_SIZES)
def test_launch_shapes_reach_both_sides_of_a_block(J):
    lay, jobs, steps, res = oracle_case(f"launch-{J}")
    assert jobs.num_jobs == J
    first = lambda j: int(jobs.step_offsets[j])
    if J >= se.BLOCK:
        assert res.scheduled[first(se.BLOCK - 1)], "the last job of block 0 schedules nothing"
    if J > se.BLOCK:
        assert res.scheduled[first(se.BLOCK)], "the first job of block 1 schedules nothing"
    if J > 2 * se.BLOCK:
        assert res.scheduled[first(2 * se.BLOCK - 1)] and res.scheduled[first(2 * se.BLOCK)]
    if J > 5:
        assert jobs.node_offsets[5] == jobs.node_offsets[6] and jobs.step_offsets[6] - jobs.step_offsets[5] == 1
        assert not res.scheduled[first(5)], "a step of a job without nodes was scheduled"
        assert (np.diff(jobs.step_offsets.astype(np.int64)) == 0).any(), "no job without steps"


def test_launch_shapes_without_steps():
    lay, jobs, steps, res = oracle_case("launch-no-steps")
    assert jobs.num_jobs == 3 and steps.num_steps == 0
    assert np.array_equal(res.avail_cpu_raw[:jobs.num_nodes], jobs.avail_cpu_raw)
