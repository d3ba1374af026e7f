"""The seam cases of the what-if probes (tests/probe_seams.py; tests/test_probe_seams.py asserts on the CPU that each one sits on its
seam) on the engine.  For every case: the cycle equals the oracle's (helpers.assert_same); the probe answers equal
tests/probe_case.expected in every field (start_sec, reason, node_idx, ntasks, cpu_raw, mem, the core planes, gres); they come out
the same a second time; the cycle's download, the costs and the seam nodes' time maps are unchanged behind the probes.  Families R-A,
R-C, R-D, S, K, T, U, V run under every kernel fixture (R-A and R-C also under CNS_SELECT_KERNEL=mem), a case of R-B under its
case's kernel word, family D everywhere — and cns_debug_get_dips must show the dip the case is about at node 0's slot before the
probes run (check_dip: a reservation's dip under every kernel, `legacy` included; a refused queue job's under the kernels that store
theirs): without it the case would test nothing, so it fails, it does not skip.  The two dip_name_* cases carry NO dip assertion under
any kernel — k_wide stores no dip for a refusal by a name's total alone —: behind a queue job they are plain parity, and only their
rdip_name_* twins show that the name-total part of the filter was exercised.  No tolerances: everything is integer or
bit-exact.  The expected answers are computed once per case and shared by the fixtures.  The hand-made cases are one test each; the
replays of the select suite (1201 cases) run as one test per family and kernel word, which names every case whose answers differ."""
import numpy as np
import pytest

from tests import helpers
from tests import probe_case as pc
from tests import probe_seams as ps
from tests.test_gpu_probe import _assert_probes
from tests.test_gpu_select_seams import FIELDS

pytestmark = pytest.mark.gpu
SHAPE = ps.SHIPPED
NO_DIP = 0xFFFFFFFF


@pytest.fixture(scope="module")
def expected_of(built):
    """(family, name) -> (case, the oracle's run of the cycle, the expected probe answers): computed once, shared by the kernel
    fixtures and left unchanged.  Family R-B's clusters are large and each is used once: not kept."""
    from cranesched_amd import engine
    from oracle import pyoracle
    assert engine.probe_shape() == SHAPE and engine.select_shape() == ps.SEL
    memo = {}

    def get(family, name):
        if (family, name) in memo:
            return memo[family, name]
        case = ps.case(SHAPE, family, name)
        kw = dict(running=case.running, reservations=case.reservations, **case.cfg)
        runs = ps.memo_of(case)      # (the replays of one select case share their prefixes: every distinct queue is run once)
        cycle = runs.select(case.queue) if runs is not None else pyoracle.select(case.cluster, case.queue, case.now, **kw)
        got = (case, cycle, pc.expected(case.cluster, case.queue, case.probes, case.now, memo=runs, **kw))
        if family != "RB":
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


def maps_of(eng, case):
    return {n: eng.timeline(n) for n in case.nodes}


def same_maps(a, b, tag):
    for n in a:
        for f in FIELDS:
            assert np.array_equal(a[n][f], b[n][f]), f"{tag}: time map of node {n} differs in {f}:\n{a[n][f]}\n{b[n][f]}"


def snapshot(eng, case):
    eng.set_nodes(case.cluster)
    eng.set_reservations(case.reservations)
    eng.set_running(case.running)


# The kernels that store the dip of a refused start-now candidate to KParams::dip_* (record_dip: k_wide's scanners).  k_select and k_pipe
# keep theirs in registers and LDS: behind them a probe reads the dips k_init_nodes posted, and nothing else.
POSTS_QUEUE_DIPS = ("wide", "wide32", "wide16", "wide8", "mem")


def check_dip(eng, case, word, first_cycle=False):
    """cns_debug_get_dips in front of the probes: the dip the case is about is there — else the case tests nothing: it fails, it does not
    skip.  A reservation's dip (k_init_nodes) under every kernel; a refused queue job's under the kernels that post theirs."""
    slot, t, by = case.dip
    d = eng.dips()
    shown = {k: v.tolist() for k, v in d.items()}
    if case.before is not None and not first_cycle:
        lo = int(case.cluster.part_offsets[1])
        assert d["t"][lo:].tolist() == [NO_DIP] * (len(d["t"]) - lo), (case.name, word, "the earlier cycle's dips of partition 1 are still there", shown)
    elif by == "resv" or (by == "queue" and word in POSTS_QUEUE_DIPS):
        assert int(d["t"][slot]) == t, (case.name, word, "no dip at the slot the probes read", shown)


def run_case(eng, case, ref, exp, kernel=None, word=None):
    snapshot(eng, case)
    if case.before is not None:          # an earlier cycle on the handle: what it left must not show
        eng.node_select(case.now, case.before)
        check_dip(eng, case, word, first_cycle=True)
    cycle = eng.node_select(case.now, case.queue)
    whole = case.before is None and case.queue.num_jobs > 0
    if whole:
        helpers.assert_same(eng, cycle, ref, case.cluster, tag=case.name)
        same_maps(maps_of(eng, case), {n: ref.timeline(n) for n in case.nodes}, case.name + ", against the oracle")
    else:                                # (the oracle builds no node of a partition without a job: the placements only)
        assert cycle.diff(ref.placements) is None, case.name
    if kernel is not None:
        k = eng.last_kernel()
        assert k.startswith(kernel[1][0]) and k.endswith(kernel[1][1]), (case.name, k, kernel)
    if case.dip is not None:
        check_dip(eng, case, word)
    costs, maps = eng.costs().view(np.uint64).copy(), maps_of(eng, case)
    first = eng.probe(case.probes)
    _assert_probes(f"{case.name} behind {eng.last_kernel()}", first, exp, case.probes)
    again = eng.probe(case.probes)
    assert first.diff(again) is None, f"{case.name}: the second probe call differs from the first"
    # nothing is committed
    assert np.array_equal(costs, eng.costs().view(np.uint64)), case.name
    same_maps(maps, maps_of(eng, case), case.name + ", behind the probes")
    assert eng.download().diff(cycle) is None, f"{case.name}: the cycle's download changed behind the probes"
    return first


def plain(fams):
    return [(f, n) for f in fams for n in ps.case_names(SHAPE, f)]


HAND = plain(("S", "K", "T", "D", "U", "V"))
REPLAYS = ("RA", "RC", "RD")


def run_family(eng_of, expected_of, family, word):
    """Every case of a replay family under one kernel word, in one test: the cases are hundreds of tiny cycles that differ in one
    job (a few milliseconds each).  A case whose answers differ (AssertionError) is written down, in full, and the next one runs: the
    failures come out together, by name.  Anything else — an error of the engine, a device fault, a failed launch — ends the test
    at once: nothing more is started on the device behind it."""
    failed = []
    for name in ps.case_names(SHAPE, family):
        case, ref, exp = expected_of(family, name)
        try:
            run_case(eng_of(case.cfg), case, ref, exp, word=word)
        except AssertionError as e:
            failed.append(f"{name}: {e}")
    assert not failed, f"{len(failed)} of {len(ps.case_names(SHAPE, family))} cases of {family} fail under {word}:\n" + "\n".join(failed)


@pytest.mark.parametrize("family,name", HAND)
def test_seam(engine_cls, engines, expected_of, request, family, name):
    case, ref, exp = expected_of(family, name)
    run_case(engines(case.cfg), case, ref, exp, word=request.node.callspec.params["engine_cls"])


@pytest.mark.parametrize("family", REPLAYS)
def test_replayed_select_seams(engine_cls, engines, expected_of, request, family):
    run_family(engines, expected_of, family, request.node.callspec.params["engine_cls"])


@pytest.mark.parametrize("family,name", HAND)
def test_seam_on_the_narrow_builds(engine_cls_narrow, engines, expected_of, request, family, name):
    """k_wide's 16- and 8-wave builds."""
    case, ref, exp = expected_of(family, name)
    run_case(engines(case.cfg), case, ref, exp, word=request.node.callspec.params["engine_cls_narrow"])


@pytest.mark.parametrize("family", REPLAYS)
def test_replayed_select_seams_on_the_narrow_builds(engine_cls_narrow, engines, expected_of, request, family):
    run_family(engines, expected_of, family, request.node.callspec.params["engine_cls_narrow"])


@pytest.mark.parametrize("family", ("RA", "RC", "D"))
def test_seams_under_the_mem_switch(engine_default, engines, expected_of, monkeypatch, family):
    """CNS_SELECT_KERNEL=mem, as tests/test_gpu_select_seams.py sets it: the default choice for partitions of this size."""
    monkeypatch.setenv("CNS_SELECT_KERNEL", "mem")
    run_family(engines, expected_of, family, "mem")


@pytest.mark.parametrize("name", ps.case_names(SHAPE, "RB"))
def test_node_count_seam(engine_default, engines, expected_of, monkeypatch, name):
    """The last job of a family-B select case as the probe behind the rest, under the kernel family whose tile the case stands on."""
    case, ref, exp = expected_of("RB", name)
    monkeypatch.setenv("CNS_SELECT_KERNEL", case.kernel[0])
    assert case.kernel[1] is not None, "the widest tile + 1 of k_select alone is refused: family R-B takes no such case"
    run_case(engines(case.cfg), case, ref, exp, kernel=case.kernel)


@pytest.mark.parametrize("name", [n for n in ps.case_names(SHAPE, "K") if ps.case(SHAPE, "K", n).plan])
def test_scratch_cap(engine_default, engines, expected_of, monkeypatch, name):
    """The mixed table under CNS_PROBE_SCRATCH_CAP at two strides and at half a stride: cns_debug_get_probe_plan reports grid 2 and grid
    1 and the stride the plan routine predicts (tests/cpp/probe_plan_test.cpp holds the routine to its definition); unset, as many
    workgroups as probes reach a walk or as are resident.  The answers are unchanged."""
    case, ref, exp = expected_of("K", name)
    eng = engines(case.cfg)
    for cap, grid, stride in case.plan:
        if cap is None:
            monkeypatch.delenv("CNS_PROBE_SCRATCH_CAP", raising=False)
        else:
            monkeypatch.setenv("CNS_PROBE_SCRATCH_CAP", str(cap))
        run_case(eng, case, ref, exp)
        g, s = eng.probe_plan()
        assert s == stride and (g == grid if grid is not None else 2 < g <= case.probes.num_jobs), (cap, g, s)


def test_a_class_the_layout_does_not_define_is_refused(engine_default, engines, expected_of):
    """The reference ignores a request for a class the layout lacks (the oracle starts such a probe now); the engine refuses the whole
    table with CNS_ERR_INVALID_ARG, as cns_upload_jobs refuses such a queue (probe.h: `validates like cns_upload_jobs`), writes nothing
    and answers the next table as before."""
    from cranesched_amd.engine import EngineError
    case, ref, exp = expected_of("D", "rdip_cpu")
    eng = engines(case.cfg)
    run_case(eng, case, ref, exp, word=None)
    bad = pc.concat(pc.take(case.probes, [0]), ps.pjobs([ps.UNDEFINED_CLASS]))
    with pytest.raises(EngineError) as e:
        eng.probe(bad)
    assert e.value.status == -1 and "probe job requests an undefined GRES class" in str(e.value), str(e.value)
    _assert_probes("behind the refused table", eng.probe(case.probes), exp, case.probes)
