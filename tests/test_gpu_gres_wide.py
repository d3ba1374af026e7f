"""GRES layouts at the engine's limits on every kernel: classes of 16 to 64 slots, bit 63, names 2 and 3, 8 classes, up to 64 node
types (tests/gres_wide.py) — the HIP engine against the CPU oracle, bit for bit (placements, fp64 cost bit patterns, time maps).

Where the hot path compresses GRES counts (4-bit class counts saturating at 15, the request total capped at 15, the front predicted
after a selection) a wrong saturation rule turns a necessary filter into a wrong one: a node with 16 free slots rejected for a request
of 15 gives another node or a later start, which only a layout with big classes shows."""
import numpy as np
import pytest

from cranesched_amd import abi
from oracle import pyoracle
from tests import gres_wide as gw
from tests import helpers

pytestmark = pytest.mark.gpu

LAYOUTS = gw.NAMED + [3, 5]   # the named layouts and two random ones


def _run(engine_cls, c, j, now, run=None, tag="", resv=None, **cfg):
    eng = engine_cls(device=0, **cfg)
    try:
        eng.set_nodes(c)
        if resv is not None:
            eng.set_reservations(resv)
        if run is not None:
            eng.set_running(run)
        got = eng.node_select(now, j)
        ref = pyoracle.select(c, j, now, running=run, reservations=resv, **cfg)
        helpers.assert_same(eng, got, ref, c, sample_nodes=48, tag=tag)
        return got, eng.last_kernel()
    finally:
        eng.close()


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("seed", [0, 1])
def test_wide_gres_random(engine_cls, lay, seed):
    c, j, now, run = gw.gres_wide_case(seed, N=96, J=700, P=2, running=60, layout=lay)
    _run(engine_cls, c, j, now, run, tag=f"{lay} {seed}")


@pytest.mark.parametrize("lay", gw.NAMED)
def test_wide_gres_deep_queue(engine_cls, lay):
    """Few nodes, a deep queue: long time maps whose entries cross the 15 / 16 boundary of the big classes, most jobs backfilled."""
    c, j, now, run = gw.gres_wide_case(10, N=16, J=1500, P=1, running=20, layout=lay)
    got, _ = _run(engine_cls, c, j, now, run, tag=f"deep {lay}")
    assert (got.reason[:j.num_jobs] == abi.REASON_PRIORITY).sum() > 300


@pytest.mark.parametrize("lay", gw.NAMED)
def test_wide_gres_narrow_builds(engine_cls_narrow, lay):
    c, j, now, run = gw.gres_wide_case(2, N=128, J=900, P=3, running=80, layout=lay)
    _run(engine_cls_narrow, c, j, now, run, tag=f"narrow {lay}")


@pytest.mark.parametrize("lay", ["uneven", "one64"])
def test_wide_gres_forced_giant(engine_default, monkeypatch, lay):
    monkeypatch.setenv("CNS_SELECT_KERNEL", "giant")
    c, j, now, run = gw.gres_wide_case(20, N=256, J=1200, P=2, running=150, layout=lay)
    _, k = _run(engine_default, c, j, now, run, tag=f"giant {lay}")
    assert k.startswith("k_giant"), k


@pytest.mark.parametrize("kernel", ["giant", "mem"])
def test_wide_gres_group_wider_than_the_tile(engine_default, monkeypatch, kernel):
    """A group of partitions sharing nodes with more (partition, node) slots than k_select's tile: k_mem (=mem), or k_giant (=giant)."""
    monkeypatch.setenv("CNS_SELECT_KERNEL", kernel)
    c, j, now, run = gw.gres_wide_case(21, N=12000, J=1500, P=4, running=400, layout="uneven", lists=False)
    c, j = gw.repartition(c, j, 21, "all+subsets")
    _, k = _run(engine_default, c, j, now, run, tag=f"{kernel} group")
    assert ("k_" + kernel) in k, k


def test_wide_gres_scaled_c4_like(engine_cls):
    """~ C4 scaled (20 000 jobs x 2 048 nodes, 8 partitions) on the uneven layout: k_wide's front predictions and k_select's dips over long
    time maps of big classes."""
    c, j, now, run = gw.gres_wide_case(30, N=2048, J=20000, P=8, running=1500, layout="uneven", lists=False)
    got, _ = _run(engine_cls, c, j, now, run, tag="C4-like wide GRES")
    assert (got.reason[:j.num_jobs] == abi.REASON_PRIORITY).sum() > 1000


@pytest.mark.parametrize("kind", ["all+subsets", "chain", "random"])
@pytest.mark.parametrize("lay", ["uneven", "eight_by_8_four_names"])
def test_wide_gres_shared_nodes(engine_cls, kind, lay):
    c, j, now, run = gw.gres_wide_case(40, N=64, J=500, P=4, running=30, layout=lay)
    c, j = gw.repartition(c, j, 40, kind)
    _run(engine_cls, c, j, now, run, tag=f"shared {kind} {lay}")


@pytest.mark.parametrize("lay", gw.NAMED)
def test_wide_gres_reservations(engine_cls, lay):
    c, j, now, run, rv = gw.resv_case(50, layout=lay)
    got, _ = _run(engine_cls, c, j, now, run, tag=f"resv {lay}", resv=rv)
    r = got.reason[:j.num_jobs]
    assert (r == abi.REASON_RESOURCE_RESERVED).sum() > 0 or (r == abi.REASON_RESERVATION_NOT_FOUND).sum() > 0


@pytest.mark.parametrize("tree", [None, "literal", "tiny"])
@pytest.mark.parametrize("lay", gw.NAMED)
def test_wide_gres_preemption(gpu, monkeypatch, tree, lay):
    from tests.test_preempt import compare_engine, run_engine_preempt
    if tree:
        monkeypatch.setenv("CNS_PREEMPT_TREE", tree)
    c, j, now, run, pre = gw.preempt_case(60, N=24, J=400, P=2, running=120, layout=lay)
    ref = pyoracle.select(c, j, now, running=run, preempt=pre)
    eng, pl, po = run_engine_preempt(c, j, now, run, pre)
    try:
        compare_engine(f"preempt {lay} {tree}", c, j, ref, eng, pl, po)
        assert sum(len(x) for x in po.lists()) > 0
    finally:
        eng.close()


@pytest.mark.parametrize("seed,lay", [(1, "eight_by_8_four_names"), (2, "eight_by_8_four_names"), (3, "uneven"), (4, "one64")])
def test_wide_gres_run_limits(engine_default, seed, lay, monkeypatch):
    """GRES limits on every class and name of the layout (8 classes under 4 names), both device paths."""
    from tests.test_run_limits import _gpu_vs_oracle, random_limit_case
    case = gw.gres_wide_case(seed, N=128, J=900, P=2, running=0, layout=lay)
    for mode in ("parallel", "seq"):
        if mode == "seq":
            monkeypatch.setenv("CNS_LIMITS_MODE", "seq")
        else:
            monkeypatch.delenv("CNS_LIMITS_MODE", raising=False)
        cluster, jobs, now, lay_, t, lj = random_limit_case(seed, tight=seed % 2 == 1, case=case)
        _gpu_vs_oracle(engine_default, cluster, jobs, now, lay_, t, lj, f"limits {lay} {seed} {mode}")


@pytest.mark.parametrize("lay", LAYOUTS)
def test_wide_gres_steps(engine_default, lay):
    from tests import kat
    l, jobs, steps = gw.step_case(7, layout=lay, J=600)
    eng = engine_default(device=0)
    try:
        eng.set_nodes(kat.cluster([4], layout=l))
        got, _ = eng.schedule_steps(jobs, steps)
        ref = pyoracle.schedule_steps(l, jobs, steps)
        assert got.diff(ref) is None, got.diff(ref)
    finally:
        eng.close()


def test_wide_gres_group_over_one_device_twice(gpu):
    from cranesched_amd.engine import GpuNodeSelectorGroup
    c, j, now, run = gw.gres_wide_case(70, N=256, J=2000, P=4, running=100, layout="eight_by_8_four_names")
    ref = pyoracle.select(c, j, now, running=run)
    g = GpuNodeSelectorGroup([0, 0])
    try:
        g.set_nodes(c)
        g.set_running(run)
        got = g.node_select(now, j)
        assert got.diff(ref.placements) is None, got.diff(ref.placements)
    finally:
        g.close()


@pytest.mark.parametrize("lay", ["uneven", "eight_by_8_four_names"])
def test_exactly_64_node_types(engine_cls, lay):
    """64 distinct res_total records: node type id 63 and bit 63 of every job's type mask; every partition is served."""
    c, j, now, run = gw.gres_wide_case(80, N=160, J=900, P=2, running=60, layout=lay, types=64)
    assert gw.num_types(c) == abi.MAX_NODE_TYPES
    eng = engine_cls(device=0)
    try:
        eng.set_nodes(c)
        eng.set_running(run)
        got = eng.node_select(now, j)
        assert (eng.partition_status() == abi.PART_SERVED).all(), eng.partition_status()
        ref = pyoracle.select(c, j, now, running=run)
        helpers.assert_same(eng, got, ref, c, sample_nodes=64, tag=f"64 types {lay}")
    finally:
        eng.close()
