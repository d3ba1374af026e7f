"""The seam cases of the what-if probes (tests/probe_seams.py) on the CPU: every case's CONDITION — what puts it on its seam — holds on
the oracle's own answers (tests/probe_case.expected: one oracle cycle over queue + [probe]) and, where oracle/_ref is built, on the
reference's own NodeSelect; the case list covers every field of cns_probe_shape; every probe table holds a probe that starts now and
one that does not, except where the case says why it cannot.  tests/test_gpu_probe_seams.py holds the engine to the same answers."""
import numpy as np
import pytest

from tests import probe_case as pc
from tests import probe_seams as ps
from tests.test_select_seams import oracle_runner

SHAPE = ps.SHIPPED
_RUNNERS = {}     # (select case, backend) -> its oracle_runner: the replays of one select case share its runs


class Ctx:
    """What a CONDITION reads: the oracle's answers, never the engine's."""

    def __init__(self, case, backend="oracle"):
        from oracle import pyoracle
        self.case, self.probes, self.backend = case, case.probes, backend
        kw = dict(running=case.running, reservations=case.reservations, backend=backend, **case.cfg)
        memo = ps.memo_of(case)      # (every distinct queue on a snapshot is run once per backend: the replays share their prefixes)
        self.run = (lambda jobs: memo.select(jobs, backend)) if memo is not None else (lambda jobs: pyoracle.select(case.cluster, jobs, case.now, **kw))
        self.cycle = self.run(case.queue)
        self.exp = pc.expected(case.cluster, case.queue, case.probes, case.now, memo=memo, **kw)

    def answer(self, i):
        return ps.answer(self.exp, self.probes, i)

    def select_ora(self, sc):
        key = (id(sc.cluster), self.backend)
        if key not in _RUNNERS:
            _RUNNERS[key] = (sc, oracle_runner(sc, backend=self.backend))
        return _RUNNERS[key][1]


def expected_of(case, backend="oracle"):
    return Ctx(case, backend)


def check_case(case):
    from oracle import pyoracle
    ctx = Ctx(case)
    seen = case.condition(ctx)
    assert isinstance(seen, dict) and seen
    Q = case.probes.num_jobs
    now = sum(1 for i in range(Q) if ps.starts_now(ctx.answer(i)))
    if case.one_sided is None:
        assert 0 < now < Q, (case.name, "the table must hold a probe that starts now and one that does not", now, Q)
    else:
        assert isinstance(case.one_sided, str) and len(case.one_sided) > 20
    if pyoracle.ref_available() and not case.cfg:   # (the reference's limits are compile-time constants: not the cases with a configured one)
        ref = Ctx(case, backend="ref")
        assert ref.exp.diff(ctx.exp) is None, case.name
        case.condition(ref)
    return seen


def test_the_case_lists_are_built_for_the_shapes_the_library_exports(built):
    from cranesched_amd import engine
    assert engine.probe_shape() == SHAPE and engine.select_shape() == ps.SEL


def test_the_cases_cover_every_field_of_the_shape():
    covered, names = set(), []
    for fam in ps.FAMILIES:
        for name in ps.case_names(SHAPE, fam):
            names.append(name)
            if fam not in ("RB",):
                covered |= set(ps.case(SHAPE, fam, name).covers)
    assert covered == set(SHAPE._fields), set(SHAPE._fields) ^ covered
    assert len(set(names)) == len(names)
    b = SHAPE.block
    for N in (b - 1, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 1):
        for s in (0, b - 1, b, N - 1):
            assert s >= N or f"only_n{N}_s{s}" in names, (N, s)
    n = 2 * b + 1
    for k in (b - 1, b, b + 1, 2 * b, 2 * b + 1):
        assert f"k{k}_n{n}_idle" in names and f"k{k}_n{n}_busy" in names, k
    for n_p in (3, b + 1):
        for k in (n_p - 1, n_p, n_p + 1):
            assert f"k{k}_n{n_p}_idle" in names and f"k{k}_n{n_p}_busy" in names, (n_p, k)
    # family R takes every case of the select suite's families A and C, twice where a job follows the decisive one
    from tests import select_seams as ss
    for fam in "AC":
        for sname in ss.case_names(ps.SEL, fam):
            assert f"{sname}__d" in names, sname
            assert f"{sname}__f" in names or sname.startswith("cap_"), sname
    assert len(ss.case_names(ps.SEL, "A")) == 270 and len(ss.case_names(ps.SEL, "C")) == 20
    sat = SHAPE.dip_gres_sat
    assert all(f"dip_gres_free{f}" in names for f in (sat - 1, sat, sat + 1, sat + 2))


@pytest.mark.parametrize("family,name", [(f, n) for f in ("S", "K", "T", "D", "U", "V") for n in ps.case_names(SHAPE, f)])
def test_case_meets_its_condition(built, family, name):
    check_case(ps.case(SHAPE, family, name))


@pytest.mark.parametrize("family,name", [(f, n) for f in ("RA", "RC", "RD", "RB") for n in ps.case_names(SHAPE, f)])
def test_replayed_select_case_meets_its_condition(built, family, name):
    check_case(ps.case(SHAPE, family, name))


def test_the_generators_are_deterministic():
    for fam in ("S", "K", "T", "D", "U", "V"):
        kept = [ps.case(SHAPE, fam, n) for n in ps.case_names(SHAPE, fam)]
        fresh = ps.FAMILIES[fam](SHAPE)
        assert [c.name for c in kept] == [c.name for c in fresh]
        for a, b in zip(kept, fresh):
            for f in ("partition", "time_limit_sec", "task_cpu_raw", "task_mem", "node_num", "ntasks", "gres_total", "gres_spec"):
                assert np.array_equal(getattr(a.probes, f), getattr(b.probes, f)) and np.array_equal(getattr(a.queue, f), getattr(b.queue, f)), (a.name, f)
            assert np.array_equal(a.cluster.cpu_total_raw, b.cluster.cpu_total_raw) and np.array_equal(a.cluster.mem_total, b.cluster.mem_total)
            assert a.nodes == b.nodes and a.covers == b.covers and a.dip == b.dip and a.plan == b.plan


def test_the_reference_ignores_a_class_the_layout_does_not_define(built):
    """... which is why that request is no case of family D: the engine refuses it (tests/test_gpu_probe_seams.py), the oracle starts it."""
    case = ps.case(SHAPE, "D", "rdip_cpu")
    one = case._replace(probes=ps.pjobs([ps.UNDEFINED_CLASS]))
    assert ps.starts_now(Ctx(one).answer(0))
