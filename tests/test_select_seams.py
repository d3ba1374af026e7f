"""The seam cases of the selection kernels (tests/select_seams.py) on the CPU: every case's CONDITION — what puts it on its seam — holds
on the oracle's own answers, the reference build (where there is one) places every job as the oracle does, the generators are
deterministic, and the case list covers every field of cns_select_shape.  tests/test_gpu_select_seams.py holds the engine to the
oracle on the same cases."""
import dataclasses

import numpy as np
import pytest

from tests import kat
from tests import select_seams as ss

SHAPE = ss.SHIPPED
NO_NODE_FITS = [dict(cpu=100000, L=1)]   # the queue "in front of the first job": one job no node's total fits, nothing is committed


def oracle_runner(case, backend="oracle"):
    """ora(n): the oracle's run of the first n jobs of the case's queue (None: all of it), each computed once."""
    from oracle import pyoracle
    memo = {}

    def ora(n=None):
        if n not in memo:
            specs = case.specs if n is None else (case.specs[:n] or NO_NODE_FITS)
            memo[n] = pyoracle.select(case.cluster, kat.jobs(specs), case.now, running=case.running, backend=backend, **case.cfg)
        return memo[n]
    return ora


def test_the_case_lists_are_built_for_the_shape_the_library_exports(built):
    from cranesched_amd import engine
    assert engine.select_shape() == SHAPE


def test_the_case_names_cover_every_field_of_the_shape():
    """A constant of the shape without a case fails; so does a tile of a kernel family without its three partitions."""
    covered = set()
    names = []
    for fam in ss.FAMILIES:
        for c in ss.cases(SHAPE, fam).values():
            covered |= set(c.covers)
            names.append(c.name)
    assert covered == set(SHAPE._fields), set(SHAPE._fields) ^ covered
    assert len(set(names)) == len(names)
    c = SHAPE.tl_chunk
    for M in (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1):
        for kind in ("win", "spoil", "run", "t0", "excl"):
            assert any(n.startswith(f"{kind}_M{M}_") for n in names), (kind, M)
    for k in (SHAPE.multi_k, SHAPE.multi_k + 1, SHAPE.max_upd, SHAPE.max_upd + 1, SHAPE.lds_heap):
        assert all(f"k{k}_{kind}" in names for kind in ("now", "bf", "nt", "ntbf", "excl")), k
    for r in (SHAPE.pipe_ring, SHAPE.wide_task_ring, SHAPE.wide_window, SHAPE.pipe_xring):
        assert all(f"burst_{n}_on{nodes}{mid}" in names for n in (r - 1, r, r + 1, 2 * r + 1) for nodes in (1, 2) for mid in ("", "_mid")), r
    tiles = [("select", SHAPE.select), ("pipe", SHAPE.pipe)] + [(f"wide{w}", t) for w, t in SHAPE.wide]
    for tag, t in tiles:
        for w in t.widths:
            for N in (t.lanes * w - 1, t.lanes * w, t.lanes * w + 1):
                assert f"one_{tag}_w{w}_n{N}" in names and f"multi_{tag}_w{w}_n{N}" in names, (tag, w, N)
    other = SHAPE._replace(tl_chunk=32, multi_k=4, max_upd=16, lds_heap=20, pipe_ring=16)
    assert {"win_M65_e32", "k4_now", "k17_bf", "k19_nt", "k20_excl", "burst_17_on1"} <= {n for f in "ACD" for n in ss.case_names(other, f)}


def same_arrays(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y), f.name
    return True


def same_case(case, rebuilt):
    assert same_arrays(case.cluster, rebuilt.cluster) and same_arrays(case.jobs, rebuilt.jobs) and case.specs == rebuilt.specs and case.cfg == rebuilt.cfg
    assert (case.running is None) == (rebuilt.running is None) and (case.running is None or same_arrays(case.running, rebuilt.running))
    assert case.nodes == rebuilt.nodes and case.covers == rebuilt.covers and case.kernel == rebuilt.kernel
    return True


def check_case(case, rebuilt=None):
    from oracle import pyoracle
    ora = oracle_runner(case)
    seen = case.condition(ora)
    assert isinstance(seen, dict) and seen
    assert rebuilt is None or same_case(case, rebuilt)
    if pyoracle.ref_available() and not case.cfg:   # the reference's own code places every job as the oracle does (its limits are compile-time constants: not the cases with a configured one)
        ref = oracle_runner(case, backend="ref")()
        assert ref.placements.diff(ora().placements) is None, case.name
        for n in case.nodes[:4]:
            a, b = ref.timeline(int(n)), ora().timeline(int(n))
            assert all(np.array_equal(a[f], b[f]) for f in a), (case.name, n)
    return seen


@pytest.mark.parametrize("name", ss.case_names(SHAPE, "A"))
def test_time_map_case_meets_its_condition(built, name):
    check_case(ss.case(SHAPE, "A", name))


@pytest.mark.parametrize("name", ss.case_names(SHAPE, "B"))
def test_node_count_case_meets_its_condition(built, name):
    check_case(ss.case(SHAPE, "B", name), ss.case(SHAPE, "B", name))


@pytest.mark.parametrize("name", ss.case_names(SHAPE, "C"))
def test_node_num_case_meets_its_condition(built, name):
    check_case(ss.case(SHAPE, "C", name))


@pytest.mark.parametrize("name", ss.case_names(SHAPE, "D"))
def test_ring_and_cache_case_meets_its_condition(built, name):
    check_case(ss.case(SHAPE, "D", name))


@pytest.mark.parametrize("family", ["A", "C", "D"])
def test_the_generators_are_deterministic(family):
    """(family B: every case is built twice in its own test above)"""
    kept = ss.cases(SHAPE, family)
    fresh = {c.name: c for c in ss.FAMILIES[family](SHAPE)}
    assert list(kept) == list(fresh) and all(same_case(kept[n], fresh[n]) for n in kept)


def test_the_serving_kernel_follows_the_plan():
    """ss.serving_kernel against the rows tests/cpp/plan_host_test.cpp pins for one partition."""
    assert ss.serving_kernel(SHAPE, 64, 8193) == ("k_wide<4>", "x64") and ss.serving_kernel(SHAPE, 64, 2049) == ("k_wide<1>", "x64")
    assert ss.serving_kernel(SHAPE, "pipe", 2049) == ("k_pipe<8>", "") and ss.serving_kernel(SHAPE, "select", 2049) == ("k_select<10>", "")
    assert ss.serving_kernel(SHAPE, "pipe", 8193) == ("k_select<19>", "") and ss.serving_kernel(SHAPE, 16, 8193) == ("k_select<19>", "")
    assert ss.serving_kernel(SHAPE, 8, 4097) == ("k_pipe<16>", "") and ss.serving_kernel(SHAPE, 32, 16385) == ("k_select<37>", "")
    assert ss.serving_kernel(SHAPE, "select", 448 * 37 + 1) is None and ss.serving_kernel(SHAPE, 64, 65537) == ("k_", "slots")
