"""The seam cases of TryPreempt_'s device form (tests/preempt_seams.py; tests/test_preempt_seams.py asserts on the CPU that each one sits
on its seam) on the engine: placements, preempted lists in push-back order, cancelled ids, the preempting set, the fp64 costs as bits and
every node's final time map must equal the oracle's — twice on one handle.  No debug setting is involved: the compressed trees run out at
their shipped capacity, the pool at its shipped size."""
import pytest

from tests import preempt_seams as ps
from tests.test_preempt import compare_engine

pytestmark = pytest.mark.gpu
RESIDENT = ["nc_257", "multi_k3", "compact_over"]


@pytest.fixture(scope="module")
def shape(built):
    from cranesched_amd import engine
    return engine.preempt_shape()


@pytest.fixture(scope="module")
def oracle_of(shape):
    """name -> (case inputs, the oracle's run): computed once, shared by the tests below and left unchanged."""
    memo = {}

    def get(name):
        if name not in memo:
            from oracle import pyoracle
            c, j, now, run, pre = ps.case(shape, name).inputs
            memo[name] = ((c, j, now, run, pre), pyoracle.select(c, j, now, running=run, preempt=pre))
        return memo[name]
    return get


def engine_for(c, run):
    from cranesched_amd.engine import GpuNodeSelector
    eng = GpuNodeSelector(device=0)
    eng.set_nodes(c)
    eng.set_running(run)
    return eng


@pytest.mark.parametrize("name", [n for n in ps.CASE_NAMES if n != "pool_over"])
def test_seam_case(gpu, oracle_of, name):
    (c, j, now, run, pre), ref = oracle_of(name)
    assert sum(len(x) for x in ref.preempt_out.lists()) > 0, "a condition on the inputs: the case preempts"
    eng = engine_for(c, run)
    try:
        first = eng.node_select_preempt(now, j, pre)
        compare_engine(name, c, j, ref, eng, *first)
        assert eng.last_kernel().startswith("k_select"), eng.last_kernel()
        again = eng.node_select_preempt(now, j, pre)
        compare_engine(name + ", again", c, j, ref, eng, *again)
        assert first[0].diff(again[0]) is None and first[1].lists() == again[1].lists() and eng.last_kernel().startswith("k_select")
    finally:
        eng.close()


def test_a_call_past_the_pool_is_refused_and_the_next_one_served(gpu, shape, oracle_of):
    """pool_over: the call's trees need more nodes than the per-partition pool holds.  The kernel notes that and ends as always (nothing
    is written once the pool is full, every walk stops): the call returns CNS_ERR_UNSUPPORTED and names the job and the pool.  The
    next call on the handle — nc_65, another cluster — is exact."""
    from cranesched_amd.engine import EngineError
    (c, j, now, run, pre), _ = oracle_of("pool_over")
    eng = engine_for(c, run)
    try:
        with pytest.raises(EngineError) as e:
            eng.node_select_preempt(now, j, pre)
        assert e.value.status == -4, str(e.value)   # CNS_ERR_UNSUPPORTED
        assert f"job {j.num_jobs - 1} needs more segment-tree nodes than the per-partition pool ({shape.pool_nodes}) holds" in str(e.value), str(e.value)
        (c2, j2, now2, run2, pre2), ref2 = oracle_of(f"nc_{shape.sort_lanes + 1}")
        eng.set_nodes(c2)
        eng.set_running(run2)
        pl, po = eng.node_select_preempt(now2, j2, pre2)
        compare_engine("after the refusal", c2, j2, ref2, eng, pl, po)
    finally:
        eng.close()


@pytest.mark.parametrize("name", RESIDENT)
def test_seam_case_on_the_resident_running_set(gpu, oracle_of, name):
    """The same answers from cns_running_select_preempt on a seeded ledger (and the index it builds there)."""
    from tests.test_gpu_running_preempt import check_case
    (c, j, now, run, pre), _ = oracle_of(name)
    eng, _, ref = check_case(name, c, j, now, run, pre)
    try:
        assert eng.last_kernel().startswith("k_select")
    finally:
        eng.close(); ref.close()
