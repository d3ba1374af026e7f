"""The seam cases of the selection kernels (tests/select_seams.py; tests/test_select_seams.py asserts on the CPU that each one sits on
its seam) on the engine: placements, reasons, starts, the fp64 costs as bit patterns (helpers.assert_same) and the final time map of
every seam node, entry for entry, must equal the oracle's — twice on one handle, the second cycle equal to the first.  Families A, C
and D run under every kernel fixture (A and C also on k_mem); a case of family B runs under the kernel family whose tile it stands on,
and last_kernel() must name the instantiation the shape predicts.  No tolerances: everything is integer or bit-exact."""
import numpy as np
import pytest

from tests import helpers
from tests import select_seams as ss

pytestmark = pytest.mark.gpu
SHAPE = ss.SHIPPED
FIELDS = ("t", "cpu_raw", "mem", "core_lo", "core_hi", "gres", "core_w2", "core_w3")


@pytest.fixture(scope="module")
def oracle_of(built):
    """(family, name) -> (case, the oracle's run): computed once, shared by the kernel fixtures and left unchanged.  Family B's
    clusters are large and each is used once: not kept."""
    from cranesched_amd import engine
    from oracle import pyoracle
    assert engine.select_shape() == SHAPE
    memo = {}

    def get(family, name):
        if (family, name) in memo:
            return memo[family, name]
        case = ss.case(SHAPE, family, name)
        got = (case, pyoracle.select(case.cluster, case.jobs, case.now, running=case.running, **case.cfg))
        if family != "B":
            memo[family, name] = got
        return got
    return get


@pytest.fixture(scope="module")
def engines(built):
    """One handle per configuration for the whole module (CNS_SELECT_KERNEL is read at every run, a snapshot replaces the one before)."""
    from cranesched_amd.engine import GpuNodeSelector
    made = {}

    def get(cfg):
        key = tuple(sorted(cfg.items()))
        if key not in made:
            made[key] = GpuNodeSelector(device=0, **cfg)
        return made[key]
    yield get
    for e in made.values():
        e.close()


def same_maps(eng, ref, case, tag):
    for n in case.nodes:
        a, b = eng.timeline(int(n)), ref.timeline(int(n))
        for f in FIELDS:
            assert np.array_equal(a[f], b[f]), f"{tag}: time map of node {n} differs in {f}:\n{a[f]}\n{b[f]}"


def run_case(eng, case, ref, kernel=None):
    eng.set_nodes(case.cluster)
    eng.set_running(case.running)
    first = eng.node_select(case.now, case.jobs)
    helpers.assert_same(eng, first, ref, case.cluster, tag=case.name)
    same_maps(eng, ref, case, case.name)
    if kernel is not None:
        k = eng.last_kernel()
        assert k.startswith(kernel[0]) and k.endswith(kernel[1]), (case.name, k, kernel)
    again = eng.node_select(case.now, case.jobs)
    assert first.diff(again) is None, f"{case.name}: the second cycle on the handle differs from the first"
    helpers.assert_same(eng, again, ref, case.cluster, tag=case.name + ", again")
    same_maps(eng, ref, case, case.name + ", again")


ACD = [(f, n) for f in "ACD" for n in ss.case_names(SHAPE, f)]


@pytest.mark.parametrize("family,name", ACD)
def test_seam(engine_cls, engines, oracle_of, family, name):
    case, ref = oracle_of(family, name)
    run_case(engines(case.cfg), case, ref)


@pytest.mark.parametrize("family,name", ACD)
def test_seam_on_the_narrow_builds(engine_cls_narrow, engines, oracle_of, family, name):
    """k_wide's 16- and 8-wave builds."""
    case, ref = oracle_of(family, name)
    run_case(engines(case.cfg), case, ref)


@pytest.mark.parametrize("family,name", [(f, n) for f in "AC" for n in ss.case_names(SHAPE, f)])
def test_seam_under_the_mem_switch(engine_default, engines, oracle_of, monkeypatch, family, name):
    """CNS_SELECT_KERNEL=mem, as tests/test_gpu_giant.py sets it.  The word moves only the shapes of k_giant to k_mem (plan_host.inc);
    partitions of this size stay on the default choice — the one setting the four words of engine_cls never take: the widest k_wide
    build that fits, with its windows and extra home workgroup as the queue decides, and kernel_pin ignored."""
    monkeypatch.setenv("CNS_SELECT_KERNEL", "mem")
    case, ref = oracle_of(family, name)
    run_case(engines(case.cfg), case, ref, kernel=("k_wide<1>", "x64"))


@pytest.mark.parametrize("name", ss.case_names(SHAPE, "B"))
def test_node_count_seam(engine_default, engines, oracle_of, monkeypatch, name):
    """Under the kernel family the case is built for; where the partition is wider than the family's widest tile, the kernel that
    serves instead — or, for k_select alone (CNS_SELECT_KERNEL=legacy), the refusal."""
    from cranesched_amd.engine import EngineError
    case, ref = oracle_of("B", name)
    word, kernel = case.kernel
    monkeypatch.setenv("CNS_SELECT_KERNEL", word)
    eng = engines(case.cfg)
    if kernel is None:
        eng.set_nodes(case.cluster)
        eng.set_running(None)
        with pytest.raises(EngineError) as e:
            eng.node_select(case.now, case.jobs)
        assert e.value.status == -4 and "widest register tile" in str(e.value), str(e.value)   # CNS_ERR_UNSUPPORTED
        return
    run_case(eng, case, ref, kernel=kernel)
